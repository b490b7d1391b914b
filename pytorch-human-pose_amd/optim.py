"""Optimizers whose step is one HIP launch (csrc/optim.hip): `Adam`, `AdamW`, `SGD`, the `GradScaler` that goes with them, and
`create_optimizer`, the counterpart of the reference's utils/optim.py:40-45.

The classes subclass torch.optim.Optimizer with torch's constructor arguments and defaults and keep torch's state format
(`step`, `exp_avg`, `exp_avg_sq` / `momentum_buffer`), so param groups, LR schedulers, `state_dict()` / `load_state_dict()` and a
hand-over to or from `torch.optim.Adam(capturable=True)` / `torch.optim.SGD` work as usual.  What they do not cover raises ValueError:
amsgrad, maximize, differentiable, dampening != 0, sparse gradients, parameters that are not fp32 on one GPU.

`_step_supports_amp_scaling = True`: a torch.amp.GradScaler hands `grad_scale` / `found_inf` to step() and never reads them on the
host; a step with non-finite gradients is skipped on the device.  `GradScaler` below replaces the scaler's foreach non-finite check
by one launch over the same table.  There is no fall-back to torch kernels.

Between the backward and the step (csrc/grad_stats.hip): `clip_grad_norm_(optimizer, max_norm)` is torch.nn.utils.clip_grad_norm_ over
the same table, and `optimizer.grad_stats()` gives per-parameter l2 / max / mean |grad| and the count of non-finite elements -- one
read of the gradients for both, and none at all after `GradScaler.unscale_`, whose launch leaves the statistics behind.

`ModelEMA` (csrc/ema.hip) keeps an exponential moving average of a net's weights.  Attached to an optimizer of this module it is
updated inside the step launch and follows the step's skip; `swap()` / `applied()` exchange weights and average in one launch.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from . import _lib

ALGO_ADAM, ALGO_ADAMW, ALGO_SGD = (_lib.const("OPTIM_" + k) for k in ("ADAM", "ADAMW", "SGD"))
UPLOAD_TENSORS, UPLOAD_GROUPS, UPLOAD_ALL = (_lib.const("OPTIM_UPLOAD_" + k) for k in ("TENSORS", "GROUPS", "ALL"))
_TENSOR, _GROUP, _EMA_ROW = (_lib.struct_dtype(k) for k in ("hh_optim_tensor", "hh_optim_group", "hh_ema_row"))

class _DeviceOptimizer(torch.optim.Optimizer):
    """What the three classes share: the descriptor table, its upkeep, and the two launches.

    Table upkeep.  The set of parameters that have a gradient decides the table's rows; while it stays the same only the gradient
    pointers are gathered per step (they change under zero_grad(set_to_none=True)), and the table is copied to the device only when a
    pointer or a hyper-parameter differs from what the device already holds.  A new set (first step, a parameter frozen or added, a
    loaded state dict) rebuilds the rows, creates missing state and checks every gradient's dtype and layout."""

    _step_supports_amp_scaling = True
    ALGO = -1
    STATE_KEYS: tuple = ()

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        devices = set()
        for group in self.param_groups:
            self._check_group(group)
            for p in group["params"]:
                if p.dtype != torch.float32 or not p.is_cuda:
                    raise ValueError(f"{type(self).__name__}: parameters must be fp32 tensors on the GPU, got {p.dtype} on {p.device}")
                if p.layout != torch.strided:
                    raise ValueError(f"{type(self).__name__}: sparse parameters are not supported")
                devices.add(p.device)
        if len(devices) > 1:
            raise ValueError(f"{type(self).__name__}: all parameters must be on one device, got {sorted(map(str, devices))}")
        self._rows = None  # the table of the current active set
        self._ema = None   # an attached ModelEMA: step() then runs the fused launch

    # ---- per-algorithm parts
    def _check_group(self, group) -> None:
        raise NotImplementedError

    def _fill_group(self, rec, group) -> None:
        raise NotImplementedError

    def _needs_state0(self, group) -> bool:
        return True

    # ---- torch.optim.Optimizer
    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        self._rows = None

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            self._check_group(group)
        self._rows = None

    # ---- the table
    def _rebuild(self, params, groups_of, mask: bytes):
        name = type(self).__name__
        dev = params[0].device
        adam = self.ALGO != ALGO_SGD
        active = [i for i, m in enumerate(mask) if m]
        for i in active:
            p, g = params[i], params[i].grad
            if g.layout != torch.strided:
                raise ValueError(f"{name}: sparse gradients are not supported")
            if g.dtype != torch.float32 or g.device != p.device:
                raise ValueError(f"{name}: gradients must be fp32 on the parameter's device, got {g.dtype} on {g.device}")
            if not p.is_contiguous() and not (p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last)):
                raise ValueError(f"{name}: parameters must be dense (contiguous or channels_last)")
            if g.stride() != p.stride() and p.numel() > 1:
                raise ValueError(f"{name}: a gradient's memory layout differs from its parameter's: strides {g.stride()} vs {p.stride()}")
        # state of the active parameters, in torch's format; the step counters of ALL parameters are views of one buffer
        if adam:
            old = [self.state[p].get("step") if p in self.state else None for p in params]
            steps = torch.zeros(len(params), dtype=torch.float32, device=dev)
            have = [i for i, s in enumerate(old) if s is not None]
            have_set = set(have)
            if have:
                vals = torch.stack([torch.as_tensor(old[i]).detach().to(device=dev, dtype=torch.float32).reshape(()) for i in have])
                steps[torch.tensor(have, device=dev)] = vals
            for i, p in enumerate(params):
                if i in have_set or mask[i]:
                    self.state[p]["step"] = steps[i]
        rows = np.zeros(len(active), dtype=_TENSOR)
        keep = [steps] if adam else []  # the state tensors the rows point into stay alive as long as the rows do
        for r, i in enumerate(active):
            p = params[i]
            st = self.state[p]
            need = self.STATE_KEYS if (adam or self._needs_state0(self.param_groups[groups_of[i]])) else ()
            for k in need:
                t = st.get(k)
                if t is None:
                    t = st[k] = torch.zeros_like(p, memory_format=torch.preserve_format)
                elif t.dtype != torch.float32 or t.device != p.device or (t.stride() != p.stride() and p.numel() > 1):
                    t = st[k] = torch.empty_like(p, memory_format=torch.preserve_format).copy_(t)  # (a state dict from elsewhere)
                keep.append(t)
            rec = rows[r]
            rec["numel"] = p.numel()
            rec["group"] = groups_of[i]
            for slot, k in zip(("state0", "state1"), need):
                rec[slot] = st[k].data_ptr()
            if adam:
                rec["step"] = st["step"].data_ptr()
        lib = _lib.load()
        ngroups = len(self.param_groups)
        nbytes = lib.hh_optim_table_bytes(rows.ctypes.data, len(rows), ngroups)
        if nbytes < 0:
            raise _lib.HHError(lib.hh_last_error().decode())
        self._rows = dict(mask=mask, active=active, rows=rows, dev=dev, nbytes=nbytes,
                          table=torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev),
                          groups=np.zeros(ngroups, dtype=_GROUP), sent_tensors=None, sent_groups=None, sent_stream=None, keep=keep,
                          params=[params[i] for i in active])
        return self._rows

    def _table(self):
        """-> (table record, upload mask) for this step's gradients and hyper-parameters; None when no parameter has a gradient."""
        params, groups_of = [], []
        for gi, group in enumerate(self.param_groups):
            ps = group["params"]
            params += ps
            groups_of += [gi] * len(ps)
        grads = [p.grad for p in params]
        mask = bytes(g is not None for g in grads)
        if not any(mask):
            return None, 0
        T = self._rows
        if T is None or T["mask"] != mask or len(T["groups"]) != len(self.param_groups):
            T = self._rebuild(params, groups_of, mask)
        rows = T["rows"]
        # the per-step gather: parameter pointers too (module.to() / p.data = ... moves them), state pointers only on a rebuild
        rows["param"] = [params[i].data_ptr() for i in T["active"]]
        rows["grad"] = [g.data_ptr() for g in grads if g is not None]
        groups = T["groups"]
        for gi, group in enumerate(self.param_groups):
            self._fill_group(groups[gi], group)
        upload = 0
        tb, gb = rows.tobytes(), groups.tobytes()
        stream = torch.cuda.current_stream(T["dev"])
        if T["sent_stream"] != stream:  # the copies of an earlier step are ordered before this one only on their own stream
            T["sent_tensors"] = T["sent_groups"] = None
            T["sent_stream"] = stream
        if T["sent_tensors"] != tb:
            upload |= UPLOAD_TENSORS
        if T["sent_groups"] != gb:
            upload |= UPLOAD_GROUPS
        T["pending"] = (tb, gb)
        return T, upload

    @staticmethod
    def _sent(T, upload) -> None:
        tb, gb = T.pop("pending")
        if upload & UPLOAD_TENSORS:
            T["sent_tensors"] = tb
        if upload & UPLOAD_GROUPS:
            T["sent_groups"] = gb

    @staticmethod
    def _scalar_ptr(t, what, dev):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or t.numel() != 1:
            raise ValueError(f"{what} must be an fp32 scalar tensor on {dev}")
        return t.data_ptr()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        T, upload = self._table()
        ema = getattr(self, "_ema", None)
        if T is None and ema is not None:  # nothing to step: the average still follows the weights, under the same skip rule
            ema.update(getattr(self, "found_inf", None))
        if T is not None:
            dev, rows, groups = T["dev"], T["rows"], T["groups"]
            scale = self._scalar_ptr(getattr(self, "grad_scale", None), "grad_scale", dev)
            found = self._scalar_ptr(getattr(self, "found_inf", None), "found_inf", dev)
            if ema is None:
                _lib.launch(dev, _lib.load().hh_optim_step, self.ALGO, rows.ctypes.data, len(rows), groups.ctypes.data, len(groups), scale, found,
                            T["table"].data_ptr(), T["nbytes"], upload)
            else:
                E, ema_upload = ema._table("step", T)
                _lib.launch(dev, _lib.load().hh_optim_step_ema, self.ALGO, rows.ctypes.data, len(rows), groups.ctypes.data, len(groups), scale,
                            found, T["table"].data_ptr(), T["nbytes"], upload, E["rows"].ctypes.data, len(E["rows"]), E["row_of"].ctypes.data,
                            ema.decay, int(ema.warmup), ema.n_averaged.data_ptr(), E["table"].data_ptr(), E["nbytes"], ema_upload)
                ema._sent(E, ema_upload)
            self._sent(T, upload)
            T["stats_fresh"] = False  # (gradient statistics of before this step are not reused after it)
        return loss

    @torch.no_grad()
    def check_grads_nonfinite(self, found_inf: torch.Tensor, inv_scale: torch.Tensor | None = None) -> None:
        """One launch over every gradient: found_inf (fp32 device scalar, zeroed by the caller) becomes 1 if any element is inf or
        NaN, and the gradients are multiplied by inv_scale in place unless it is None or holds 1 (GradScaler.unscale_).  With
        `collect_grad_stats` set (clip_grad_norm_ and grad_stats() set it, and so does a module built with max_grad_norm) the same
        read of the gradients also leaves their statistics -- of the unscaled values -- for those two to reuse; the stored bits and
        the flag are the same either way."""
        T, upload = self._table()
        if T is not None:
            dev, rows = T["dev"], T["rows"]
            upload &= UPLOAD_TENSORS
            scale, found = self._scalar_ptr(inv_scale, "inv_scale", dev), self._scalar_ptr(found_inf, "found_inf", dev)
            if self.collect_grad_stats:
                work = self._work(T)
                _lib.launch(dev, _lib.load().hh_grad_stats, rows.ctypes.data, len(rows), len(T["groups"]), scale, found, T["table"].data_ptr(),
                            T["nbytes"], upload, work.data_ptr(), T["work_bytes"])
                T["stats_fresh"], T["stats_found_inf"] = True, found_inf  # (kept alive: the clip launch reads it)
            else:
                _lib.launch(dev, _lib.load().hh_grads_nonfinite, rows.ctypes.data, len(rows), len(T["groups"]), scale, found, T["table"].data_ptr(),
                            T["nbytes"], upload)
            self._sent(T, upload)

    # ---- gradient statistics and clipping by global norm (csrc/grad_stats.hip)
    collect_grad_stats = False

    def zero_grad(self, set_to_none: bool = True) -> None:
        super().zero_grad(set_to_none)
        if self._rows is not None:
            self._rows["stats_fresh"] = False

    @staticmethod
    def _work(T):
        """the statistics workspace of this table (hh_grad_stats_bytes), allocated on first use"""
        if T.get("work") is None:
            lib = _lib.load()
            nbytes = lib.hh_grad_stats_bytes(T["rows"].ctypes.data, len(T["rows"]), len(T["groups"]))
            if nbytes < 0:
                raise _lib.HHError(lib.hh_last_error().decode())
            T["work_bytes"], T["work"] = nbytes, torch.empty(max(nbytes, 16), dtype=torch.uint8, device=T["dev"])
        return T["work"]

    def _grad_stats_pass(self, recompute: bool):
        """-> the table record with current statistics in its workspace (None when no parameter has a gradient).

        FRESH statistics are reused instead of reading the gradients again (and the table is not even gathered again).  They are fresh
        when they come from this optimizer's latest check_grads_nonfinite (GradScaler.unscale_) and there was no step(), zero_grad() or
        clip_grad_norm_ on it since.  They describe the gradients as that check stored them: unscaled, not yet clipped.  Code that
        writes to the gradients, or replaces them, between unscale_ and the clip passes recompute=True.  Anything else -- a call
        without a preceding check, or recompute=True -- runs a statistics launch of its own over the gradients as they are now."""
        self.collect_grad_stats = True
        T = self._rows
        if not recompute and T is not None and T.get("stats_fresh"):
            return T
        T, upload = self._table()
        if T is None:
            return None
        upload &= UPLOAD_TENSORS
        work, rows = self._work(T), T["rows"]
        _lib.launch(T["dev"], _lib.load().hh_grad_stats, rows.ctypes.data, len(rows), len(T["groups"]), None, None, T["table"].data_ptr(),
                    T["nbytes"], upload, work.data_ptr(), T["work_bytes"])
        T["stats_fresh"], T["stats_found_inf"] = False, None
        self._sent(T, upload)
        return T

    @staticmethod
    def _totals(T):
        return T["work"][:16].view(torch.float32)  # total_l2, total_inf, coef of the last clip, unused

    @torch.no_grad()
    def grad_stats(self, recompute: bool = False):
        """-> (params, stats): the parameters that have a gradient, in table order, and an [n, 4] fp32 device tensor with one row
        [l2 norm, max |g|, mean |g|, number of inf / NaN elements] per parameter (STAT_L2 .. STAT_NONFINITE).  Nothing is read on the
        host.  A NaN in a gradient makes its three figures NaN, an inf makes them inf.  Reuses fresh statistics (`_grad_stats_pass`
        says what fresh means; recompute=True forces a new pass over the gradients as they are now)."""
        T = self._grad_stats_pass(recompute)
        if T is None:
            dev = next((p.device for g in self.param_groups for p in g["params"]), None)
            return [], torch.zeros(0, 4, dtype=torch.float32, device=dev)
        n = len(T["rows"])
        return list(T["params"]), T["work"][16:16 + 16 * n].view(torch.float32).view(n, 4).clone()

    @torch.no_grad()
    def clip_coef(self) -> torch.Tensor:
        """the coefficient the last clip_grad_norm_ over this optimizer multiplied by (1 where it did not engage): 0-dim, on the device"""
        if self._rows is None or self._rows.get("work") is None:
            raise ValueError(f"{type(self).__name__}: no clip_grad_norm_ has run on the current table")
        return self._totals(self._rows)[2].clone()


def _refuse(name, **flags):
    for k, v in flags.items():
        if v:
            raise ValueError(f"{name}: {k}={v!r} is not supported by the device optimizer")


class _AdamBase(_DeviceOptimizer):
    STATE_KEYS = ("exp_avg", "exp_avg_sq")
    DECOUPLED = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=True, differentiable=False, fused=None):
        if isinstance(lr, torch.Tensor):
            raise ValueError(f"{type(self).__name__}: lr must be a Python number (it is read from the group at every step)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # torch's keys, so that a state dict loads into torch.optim.Adam(capturable=True): the step counters live on the device
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None, capturable=True,
                        differentiable=differentiable, fused=None, decoupled_weight_decay=self.DECOUPLED)
        super().__init__(params, defaults)

    def _check_group(self, group) -> None:
        _refuse(type(self).__name__, amsgrad=group.get("amsgrad", False), maximize=group.get("maximize", False),
                differentiable=group.get("differentiable", False))
        b1, b2 = group["betas"]
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"Invalid beta parameters: {group['betas']}")

    def _fill_group(self, rec, group) -> None:
        rec["lr"], rec["eps"], rec["weight_decay"] = float(group["lr"]), float(group["eps"]), float(group["weight_decay"])
        rec["beta1"], rec["beta2"] = float(group["betas"][0]), float(group["betas"][1])


class Adam(_AdamBase):
    """torch.optim.Adam (L2 weight decay) as one launch."""
    ALGO = ALGO_ADAM


class AdamW(_AdamBase):
    """torch.optim.AdamW (decoupled weight decay, default 1e-2) as one launch."""
    ALGO = ALGO_ADAMW
    DECOUPLED = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, **kw):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, **kw)


class SGD(_DeviceOptimizer):
    """torch.optim.SGD with weight decay, momentum and Nesterov momentum (dampening 0) as one launch.  The momentum buffer starts at
    zero, which at dampening 0 is torch's first step (buf = g) bit for bit."""
    ALGO = ALGO_SGD
    STATE_KEYS = ("momentum_buffer",)

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *, maximize=False, foreach=None,
                 differentiable=False, fused=None):
        if isinstance(lr, torch.Tensor):
            raise ValueError("SGD: lr must be a Python number (it is read from the group at every step)")
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=maximize, foreach=None,
                        differentiable=differentiable, fused=None)
        super().__init__(params, defaults)

    def _check_group(self, group) -> None:
        _refuse("SGD", maximize=group.get("maximize", False), differentiable=group.get("differentiable", False))
        if group.get("dampening", 0) != 0:
            raise ValueError(f"SGD: dampening={group['dampening']!r} is not supported by the device optimizer (only 0)")

    def _needs_state0(self, group) -> bool:
        return group["momentum"] != 0

    def _fill_group(self, rec, group) -> None:
        rec["lr"], rec["weight_decay"], rec["momentum"] = float(group["lr"]), float(group["weight_decay"]), float(group["momentum"])
        rec["nesterov"] = 1 if group["nesterov"] else 0

    def _rebuild(self, params, groups_of, mask):
        for p in params:  # torch keeps momentum_buffer = None for a parameter it has not stepped with momentum: same as absent here
            st = self.state.get(p)
            if st is not None and "momentum_buffer" in st and st["momentum_buffer"] is None:
                del st["momentum_buffer"]
        return super()._rebuild(params, groups_of, mask)


class GradScaler(torch.amp.GradScaler):
    """torch.amp.GradScaler whose non-finite check (and unscale_) over an optimizer of this module is one launch instead of the foreach
    family; any other optimizer goes through the parent.  State dict and public behaviour are the parent's.

    unscale_(optimizer) on an optimizer with `collect_grad_stats` set (clip_grad_norm_ / grad_stats() set it on first use, a module
    built with max_grad_norm at once) produces the gradient statistics in the launch that checks and unscales, at no extra read.  They
    stay FRESH -- clip_grad_norm_ and grad_stats() reuse them instead of reading the gradients again -- until the optimizer's next
    step(), zero_grad() or clip_grad_norm_; both take recompute=True to force a new pass."""

    def _unscale_grads_(self, optimizer, inv_scale, found_inf, allow_fp16):
        if not isinstance(optimizer, _DeviceOptimizer):
            return super()._unscale_grads_(optimizer, inv_scale, found_inf, allow_fp16)
        optimizer.check_grads_nonfinite(found_inf, inv_scale)
        return {found_inf.device: found_inf}


class ModelEMA:
    """Exponential moving average of a net's weights on the device (csrc/ema.hip), in place of torch.optim.swa_utils.AveragedModel(
    multi_avg_fn=get_ema_multi_avg_fn(decay)).

    The rule, per element in fp32, n = n_averaged before the update: n == 0 copies the weights' bits; otherwise
    d = min(decay, (1 + n) / (10 + n)) with warmup, decay without, in fp64, w = float32(1 - d) rounded once, ema += w * (value - ema).
    DIFFERENCES from torch: this one form serves every w (torch's lerp switches form at w >= 0.5), and a step that the optimizer skips
    on found_inf leaves the average and n_averaged alone (AveragedModel cannot see the skip, so it updates and counts).

    Averaged: every parameter of the bare net (DistributedDataParallel unwrapped), trainable or frozen, and with use_buffers=True
    every floating-point buffer (BatchNorm running statistics).  Integer buffers are never averaged.  state_dict()["model"] is a state
    dict of the net: averages where there are any, the net's own buffers of the moment of the call elsewhere (torch's use_buffers=False
    behaviour).  All averaged tensors must be dense fp32 on one GPU; anything else raises ValueError.

    With an optimizer of this module the EMA attaches itself: optimizer.step() then updates the average of every parameter it steps in
    the step launch, from the new value still in registers, and every other averaged tensor in further workgroups of the same launch;
    there is nothing else to call.  With any other optimizer call update() after its step: one launch over the same rows.  Neither
    reads the device on the host; n_averaged is a 0-dim int64 device tensor.  Pointers of the live tensors are gathered at every call
    (parameters move under .to(); buffers are replaced)."""

    def __init__(self, net: torch.nn.Module, optimizer=None, decay: float = 0.9998, warmup: bool = False, use_buffers: bool = False):
        from torch.nn.parallel import DistributedDataParallel as DDP
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:  # (NaN fails too)
            raise ValueError(f"ModelEMA: decay must lie in [0, 1], got {decay!r}")
        self.net = net.module if isinstance(net, DDP) else net
        self.decay, self.warmup, self.use_buffers = decay, bool(warmup), bool(use_buffers)
        # (owner module, key, is a buffer): the live tensor is looked up at every call
        self._slots, self._names = [], []
        seen = set()
        for prefix, mod in self.net.named_modules():
            kinds = [(mod._parameters, False)] + ([(mod._buffers, True)] if self.use_buffers else [])
            for store, is_buf in kinds:
                for key, t in store.items():
                    if t is None or id(t) in seen or (is_buf and (not t.is_floating_point() or key in mod._non_persistent_buffers_set)):
                        continue
                    seen.add(id(t))
                    self._slots.append(store)
                    self._names.append((prefix + "." if prefix else "") + key)
        self._keys = [n.rpartition(".")[2] for n in self._names]
        live = self._live()
        if not live:
            raise ValueError("ModelEMA: the net has no parameters")
        devices = {t.device for t in live}
        for name, t in zip(self._names, live):
            if t.dtype != torch.float32 or not t.is_cuda or t.layout != torch.strided:
                raise ValueError(f"ModelEMA: {name} must be a dense fp32 tensor on the GPU, got {t.dtype} on {t.device}")
            if not t.is_contiguous() and not (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)):
                raise ValueError(f"ModelEMA: {name} must be dense (contiguous or channels_last)")
        if len(devices) > 1:
            raise ValueError(f"ModelEMA: all averaged tensors must be on one device, got {sorted(map(str, devices))}")
        self.device = live[0].device
        self.averages = {name: torch.empty_like(t, memory_format=torch.preserve_format) for name, t in zip(self._names, live)}
        self.n_averaged = torch.zeros((), dtype=torch.int64, device=self.device)
        self._filled = False  # known on the host to hold averages (n_averaged != 0); read from the device outside the step only
        rows = np.zeros(len(live), dtype=_EMA_ROW)
        rows["ema"] = [self.averages[n].data_ptr() for n in self._names]
        rows["numel"] = [t.numel() for t in live]
        self._rows = rows
        self._tables: dict = {}  # one device table per entry point ("step", "update", "swap": their chunk lists differ)
        self.optimizer = None
        if optimizer is not None and is_device_optimizer(optimizer):
            if optimizer._ema is not None and optimizer._ema is not self:
                raise ValueError("ModelEMA: the optimizer already has an EMA attached")
            optimizer._ema = self
            self.optimizer = optimizer

    def adopt_average(self, name: str, tensor: torch.Tensor) -> None:
        """Keeps the average of `name` in `tensor` from now on, contents as they are: e.g. a view into one flat buffer that is
        all-reduced or written out as a whole.  Dense fp32 on the EMA's device, with the averaged tensor's shape and strides."""
        old = self.averages[name]
        if (tensor.dtype != torch.float32 or tensor.device != old.device or tensor.shape != old.shape
                or (tensor.stride() != old.stride() and old.numel() > 1)):
            raise ValueError(f"ModelEMA.adopt_average: {name} needs an fp32 tensor of shape {tuple(old.shape)}, strides {old.stride()} on {old.device}")
        self.averages[name] = tensor
        self._rows["ema"][self._names.index(name)] = tensor.data_ptr()

    def _live(self):
        return [store[key] for store, key in zip(self._slots, self._keys)]

    def _table(self, mode: str, T=None):
        """-> (table record of `mode`, upload flag) with this call's pointers gathered; `T` is the optimizer's table record ("step")."""
        rows = self._rows
        E = self._tables.get(mode)
        rebuild = E is None or E["of"] is not T
        if mode == "step" and not rebuild:
            # the step reads `value` only of the rows the optimizer does not step (its own rows carry the parameters' addresses)
            for r in E["only"]:
                rows["value"][r] = self._slots[r][self._keys[r]].data_ptr()
        else:
            # (like the optimizer's rows: checked when the step's table is built, and at every call outside the step)
            live = self._live()
            for name, t, numel in zip(self._names, live, rows["numel"]):
                if t.numel() != numel or t.dtype != torch.float32 or t.device != self.device:
                    raise ValueError(f"ModelEMA: {name} is now {tuple(t.shape)} {t.dtype} on {t.device}; the average was made for {int(numel)} "
                                     f"fp32 elements on {self.device}")
            rows["value"] = [t.data_ptr() for t in live]
        if rebuild:
            ntensors = len(T["rows"]) if T is not None else 0
            lib = _lib.load()
            nbytes = lib.hh_ema_table_bytes(rows.ctypes.data, len(rows), ntensors)
            if nbytes < 0:
                raise _lib.HHError(lib.hh_last_error().decode())
            row_of = np.full(max(ntensors, 1), -1, dtype=np.int32)
            if T is not None:  # a rebuilt optimizer table rebuilds the mapping
                mine = {id(t): r for r, t in enumerate(live)}
                row_of[:ntensors] = [mine.get(id(p), -1) for p in T["params"]]
            named = set(row_of.tolist())
            E = self._tables[mode] = dict(of=T, rows=rows, row_of=row_of, nbytes=nbytes, sent=None, sent_stream=None,
                                          only=[r for r in range(len(rows)) if r not in named],
                                          table=torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device))
        stream = torch.cuda.current_stream(self.device)
        if E["sent_stream"] != stream:
            E["sent"], E["sent_stream"] = None, stream
        E["pending"] = rows.tobytes()
        return E, int(E["sent"] != E["pending"])

    @staticmethod
    def _sent(E, upload) -> None:
        pending = E.pop("pending")
        if upload:
            E["sent"] = pending

    @torch.no_grad()
    def update(self, found_inf: torch.Tensor | None = None) -> None:
        """The stand-alone update, one launch over every averaged tensor; with found_inf (fp32 device scalar) != 0 nothing is stored."""
        E, upload = self._table("update")
        found = _DeviceOptimizer._scalar_ptr(found_inf, "found_inf", self.device)
        _lib.launch(self.device, _lib.load().hh_ema_update, E["rows"].ctypes.data, len(E["rows"]), self.decay, int(self.warmup),
                    self.n_averaged.data_ptr(), found, E["table"].data_ptr(), E["nbytes"], upload)
        self._sent(E, upload)

    def _ensure_filled(self) -> None:
        """Before any update the average IS the weights (AveragedModel starts as a copy).  The averages' storage is first written by
        the n == 0 update; whoever looks at them earlier (swap, state_dict) gets that copy made here.  One host read of n_averaged per
        call until it is non-zero; never from step() / update()."""
        if not self._filled:
            self._filled = bool(self.n_averaged.item() != 0)
            if not self._filled:
                with torch.no_grad():
                    torch._foreach_copy_([self.averages[n] for n in self._names], [t.detach() for t in self._live()])

    @torch.no_grad()
    def swap(self) -> None:
        """Exchanges the net's weights and their averages in place, one launch; twice is the identity, bit for bit.  The net is told
        (mark_dirty) so that an inference engine folds the weights it now holds."""
        self._ensure_filled()
        E, upload = self._table("swap")
        _lib.launch(self.device, _lib.load().hh_ema_swap, E["rows"].ctypes.data, len(E["rows"]), E["table"].data_ptr(), E["nbytes"], upload)
        self._sent(E, upload)
        if hasattr(self.net, "mark_dirty"):
            self.net.mark_dirty()

    @contextlib.contextmanager
    def applied(self):
        """`with ema.applied():` the net holds the averaged weights inside and its own again after."""
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    def state_dict(self) -> dict:
        self._ensure_filled()
        model = {}
        for name, t in self.net.state_dict().items():
            avg = self.averages.get(name)
            model[name] = avg if avg is not None else t.detach().clone()
        return {"model": model, "n_averaged": self.n_averaged, "decay": self.decay, "warmup": self.warmup, "use_buffers": self.use_buffers}

    @torch.no_grad()
    def load_state_dict(self, state_dict: dict) -> None:
        if bool(state_dict["use_buffers"]) != self.use_buffers:
            raise ValueError(f"ModelEMA: the state dict was made with use_buffers={state_dict['use_buffers']!r}, this EMA with {self.use_buffers!r}")
        decay = float(state_dict["decay"])
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"ModelEMA: decay must lie in [0, 1], got {decay!r}")
        model = state_dict["model"]
        missing = [n for n in self._names if n not in model]
        if missing:
            raise KeyError(f"ModelEMA: the state dict lacks the averages of {missing[:5]}{' ...' if len(missing) > 5 else ''}")
        for name in self._names:
            if tuple(model[name].shape) != tuple(self.averages[name].shape):
                raise ValueError(f"ModelEMA: {name} has shape {tuple(model[name].shape)} in the state dict, {tuple(self.averages[name].shape)} here")
        for name in self._names:
            self.averages[name].copy_(model[name])
        self.n_averaged.copy_(torch.as_tensor(state_dict["n_averaged"]).to(torch.int64).reshape(()))
        self.decay, self.warmup = decay, bool(state_dict["warmup"])
        self._filled = False


# utils/optim.py:10-18 of the reference: the three with a kernel here, the other four torch's own
optimizers = {"Adam": Adam, "AdamW": AdamW, "SGD": SGD, "Adamax": torch.optim.Adamax, "Adadelta": torch.optim.Adadelta,
              "Adagrad": torch.optim.Adagrad, "RMSprop": torch.optim.RMSprop}


def create_optimizer(net: torch.nn.Module, name: str, **params) -> torch.optim.Optimizer:
    """utils/optim.py:40-45: the named optimizer over the net's trainable parameters."""
    return optimizers[name](filter(lambda p: p.requires_grad, net.parameters()), **params)


def is_device_optimizer(optimizer) -> bool:
    return isinstance(optimizer, _DeviceOptimizer)


STAT_L2, STAT_ABSMAX, STAT_ABSMEAN, STAT_NONFINITE = 0, 1, 2, 3  # the columns of grad_stats()'s rows
NORM_L2, NORM_INF = _lib.const("GRAD_NORM_L2"), _lib.const("GRAD_NORM_INF")


def grad_stats_rows(named_parameters, params) -> dict:
    """{name: row} of grad_stats()'s `stats` for the entries of `named_parameters` (net.named_parameters(), or any iterable of
    (name, parameter)) that have a row; `params` is grad_stats()'s first result.  A logger prints per-layer mean / max |grad| with
    one copy of `stats` to the host: stats.cpu()[row, STAT_ABSMEAN], [row, STAT_ABSMAX]."""
    row = {id(p): r for r, p in enumerate(params)}
    return {name: row[id(p)] for name, p in named_parameters if id(p) in row}


def clip_grad_norm_(optimizer, max_norm: float, norm_type: float = 2.0, error_if_nonfinite: bool = False, recompute: bool = False) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ over the optimizer's parameters that have a gradient -> the total norm (before clipping), a
    0-dim fp32 tensor on the device.  norm_type is 2 or inf; anything else, or a max_norm that is negative or NaN, raises ValueError.

    A device optimizer of this module: one read of the gradients for the statistics (none where GradScaler.unscale_ has just left
    fresh ones -- `_DeviceOptimizer._grad_stats_pass` says what fresh means, recompute=True forces a new pass), and one launch that
    multiplies them by coef = max_norm / (total + 1e-6) in torch's fp32 arithmetic and stores nothing where coef >= 1.  The total is
    formed from fp64 sums in one fixed order and rounded once, so it is the correctly rounded norm up to fp64's own error and the same
    bits on every run; torch accumulates in fp32.  Nothing is read on the host, except with error_if_nonfinite=True: that is one host
    read of the total, before anything is scaled, and raises RuntimeError like torch.  DIFFERENCE from torch: after a
    GradScaler.unscale_ that found an inf / NaN the gradients are left as they are (torch multiplies them by 0 or NaN); that step is
    skipped either way.  Any other optimizer: torch's function over its parameters."""
    max_norm, norm_type = float(max_norm), float(norm_type)
    if norm_type not in (2.0, float("inf")):
        raise ValueError(f"clip_grad_norm_: norm_type {norm_type!r} is not supported (2 or inf)")
    if not max_norm >= 0.0:
        raise ValueError(f"clip_grad_norm_: max_norm must be a number >= 0, got {max_norm!r}")
    if not isinstance(optimizer, _DeviceOptimizer):
        params = [p for group in optimizer.param_groups for p in group["params"]]
        return torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type, error_if_nonfinite=error_if_nonfinite)
    with torch.no_grad():
        T = optimizer._grad_stats_pass(recompute)
        if T is None:
            dev = next((p.device for g in optimizer.param_groups for p in g["params"]), None)
            return torch.zeros((), dtype=torch.float32, device=dev)
        code = NORM_INF if norm_type != 2.0 else NORM_L2
        total = optimizer._totals(T)[code].clone()
        if error_if_nonfinite and not bool(torch.isfinite(total)):
            raise RuntimeError(f"The total norm of order {norm_type} for gradients from `parameters` is non-finite, so it cannot be clipped. "
                               "To disable this error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`")
        rows = T["rows"]
        _lib.launch(T["dev"], _lib.load().hh_grad_clip, rows.ctypes.data, len(rows), len(T["groups"]), max_norm, code,
                    _lib.ptr(T.get("stats_found_inf")), T["table"].data_ptr(), T["nbytes"], T["work"].data_ptr(), T["work_bytes"])
        T["stats_fresh"] = False  # (the gradients may have been scaled: the statistics no longer describe them)
        return total
