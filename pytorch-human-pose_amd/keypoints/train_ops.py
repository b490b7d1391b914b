"""Python face of the training building blocks (`hh_conv2d`, `hh_bn_train_*`): NHWC bf16 or fp16 activations as torch tensors
in channels_last memory format, fp32 parameters.  `train_net.py` assembles them into the net's training forward.

Every op takes the element type from its first activation, raises `HHError` when another activation of the same call has a different
one, and returns tensors of the type it was given (the `*_dt` entry points of include/hhrnet.h, where the fp16 semantics are stated)."""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _lib
from .._lib import launch as _launch, ptr as _ptr


ACT_DTYPES = {torch.bfloat16: _lib.ACT_BF16, torch.float16: _lib.ACT_F16}
PRECISION_DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}  # the names of HigherHRNet.set_train_precision / KeypointsModule(precision=)


def _nhwc(x: Tensor) -> Tensor:
    """[B,C,H,W] bf16 / fp16 tensor whose memory is NHWC (channels_last); returns it contiguous in that format."""
    if not x.is_cuda or x.dtype not in ACT_DTYPES or x.dim() != 4:
        raise _lib.HHError("expected a 4-d CUDA/HIP bfloat16 or float16 tensor: there is no CPU path")
    return x.contiguous(memory_format=torch.channels_last)


def _act(first: Tensor, *others) -> int:
    """the act_dtype of a call: that of its first activation; every other activation (None: absent) must have the same type"""
    for t in others:
        if t is not None and t.dtype != first.dtype:
            raise _lib.HHError(f"the activations of one call must share one element type: {first.dtype} and {t.dtype}")
    return ACT_DTYPES[first.dtype]


BN_BLOCKS = 256  # HH_BN_BLOCKS of csrc/kernels.h: the BatchNorm reductions write BN_BLOCKS * C * 2 partial sums into their scratch


def _conv_geometry(wshape, stride: int, data_grad: bool, H: int = 0, W: int = 0):
    """-> (mode of hh_conv2d, channels the input must have, channels of the output, Ho, Wo) for weights [cout,cin,ks,ks]"""
    cout, cin = wshape[:2]
    mode = (2 if stride == 2 else 1) if data_grad else 0
    if mode == 2:
        Ho, Wo = 2 * H, 2 * W  # dL/dx of a stride-2 conv lives on the input grid
    else:
        Ho, Wo = (H // 2, W // 2) if stride == 2 else (H, W)
    return (mode, cout, cin, Ho, Wo) if data_grad else (mode, cin, cout, Ho, Wo)


def conv2d(x: Tensor, w: Tensor, stride: int = 1, bias: Tensor | None = None, res: Tensor | None = None, relu: bool = False,
           data_grad: bool = False, pad: tuple[int, int] | None = None, packed: Tensor | None = None) -> Tensor:
    """y = act(conv(x, w) + bias (+ res)), padding (ks-1)/2.  data_grad=True: x is dL/dy of the conv with weights
    w [cout,cin,ks,ks] and this stride, and the result is dL/dx (stride 2: 3x3 only, even input sizes).
    packed: the weights of this (w, stride, data_grad) already packed by `PackedConvWeights` (w then only gives the shape)."""
    lib = _lib.load()
    x = _nhwc(x)
    B, Cx, H, W = x.shape
    cout, cin, ks, _ = w.shape
    mode, ci, co, Ho, Wo = _conv_geometry(w.shape, stride, data_grad, H, W)
    if Cx != ci:
        raise ValueError(f"conv2d: input has {Cx} channels, weights {tuple(w.shape)}, data_grad={data_grad}")
    y = torch.empty((B, co, Ho, Wo), device=x.device, dtype=x.dtype, memory_format=torch.channels_last)
    if packed is not None:
        fn, wk, tail = lib.hh_conv2d_packed_dt, packed, ()
    else:  # the kernel packs w itself, into a workspace
        nbytes = lib.hh_conv2d_workspace_bytes(cin, cout, ks, mode)
        if nbytes < 0:
            raise _lib.HHError("conv2d: no kernel family for this shape")
        ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)  # (alive until the launch is enqueued)
        fn, wk, tail = lib.hh_conv2d_dt, w.detach().to(x.device, torch.float32).contiguous(), (ws.data_ptr(),)
    if res is not None:
        res = _nhwc(res)
    if bias is not None:
        bias = bias.detach().to(x.device, torch.float32).contiguous()
    py_, px_ = pad if pad is not None else (-1, -1)
    # (the packed weights carry the type they were packed with)
    _launch(x.device, fn, _act(x, res, packed), x.data_ptr(), B, H, W, cin, wk.data_ptr(), cout, ks, stride, mode, py_, px_, _ptr(bias), _ptr(res),
            int(relu), y.data_ptr(), *tail)
    return y


def _bn_buffers(x: Tensor):
    """-> (two per-channel fp32 outputs: mean, invstd or dgamma, dbeta; the partial-sum scratch of the reductions)"""
    C = x.shape[1]
    return (torch.empty(C, device=x.device, dtype=torch.float32), torch.empty(C, device=x.device, dtype=torch.float32),
            torch.empty(BN_BLOCKS * C * 2, device=x.device, dtype=torch.float64))


def bn_train_forward(x: Tensor, gamma: Tensor, beta: Tensor, eps: float = 1e-5, res: Tensor | None = None, relu: bool = False):
    """-> (y, mean, invstd): BatchNorm2d in training mode (+ residual, + ReLU); mean / invstd feed the backward."""
    lib = _lib.load()
    x = _nhwc(x)
    B, C, H, W = x.shape
    y = torch.empty_like(x)
    mean, invstd, scratch = _bn_buffers(x)
    if res is not None:
        res = _nhwc(res)
    _launch(x.device, lib.hh_bn_train_forward_dt, _act(x, res), x.data_ptr(), B * H * W, C, gamma.float().contiguous().data_ptr(),
            beta.float().contiguous().data_ptr(), eps, _ptr(res), int(relu), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), scratch.data_ptr())
    return y, mean, invstd


def bn_train_backward(x: Tensor, y, dy: Tensor, mean: Tensor, invstd: Tensor, gamma: Tensor, relu: bool = False,
                      want_dres: bool = False, beta=None):
    """-> (dx, dgamma, dbeta, dres or None).  y = None (with beta): a BatchNorm without a residual input, the ReLU mask is
    recomputed from x (hh_bn_train_backward_plain)."""
    lib = _lib.load()
    if y is None:
        assert beta is not None and not want_dres
    x, y, dy = _nhwc(x), _nhwc(y) if y is not None else None, _nhwc(dy)
    B, C, H, W = x.shape
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    dgamma, dbeta, scratch = _bn_buffers(x)
    g = gamma.float().contiguous()
    if y is None:
        b = beta.float().contiguous()
        _launch(x.device, lib.hh_bn_train_backward_plain_dt, _act(x, dy), x.data_ptr(), dy.data_ptr(), B * H * W, C, mean.data_ptr(), invstd.data_ptr(),
                g.data_ptr(), b.data_ptr(), int(relu), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), scratch.data_ptr())
    else:
        _launch(x.device, lib.hh_bn_train_backward_dt, _act(x, y, dy), x.data_ptr(), y.data_ptr(), dy.data_ptr(), B * H * W, C, mean.data_ptr(),
                invstd.data_ptr(), g.data_ptr(), int(relu), dx.data_ptr(), _ptr(dres), dgamma.data_ptr(), dbeta.data_ptr(), scratch.data_ptr())
    return dx, dgamma, dbeta, dres


class PackedConvWeights:
    """Kernel-layout copies (bf16, or fp16 with dtype=torch.float16) of a set of conv weights, all refreshed by ONE launch (`refresh`,
    once per training step before the forward).  entries: (weight [cout,cin,ks,ks] fp32 CUDA parameter, stride, data_grad)."""

    def __init__(self, entries: list, dtype: torch.dtype = torch.bfloat16):
        import ctypes as C
        if dtype not in ACT_DTYPES:
            raise _lib.HHError(f"PackedConvWeights: dtype must be torch.bfloat16 or torch.float16, not {dtype}")
        self.dtype = dtype
        lib = _lib.load()
        self.n = len(entries)
        self.buffers: list[Tensor] = []
        self._keep = [w for w, _, _ in entries]
        shapes = (C.c_int32 * (5 * self.n))()
        dev = entries[0][0].device if entries else None
        for i, (w, stride, data_grad) in enumerate(entries):
            cout, cin, ks, _ = w.shape
            mode = _conv_geometry(w.shape, stride, data_grad)[0]
            nel = lib.hh_conv2d_packed_elems(cin, cout, ks, stride, mode)
            if nel < 0:
                raise _lib.HHError(f"no kernel family for conv weights {tuple(w.shape)} (stride {stride}, data_grad={data_grad})")
            self.buffers.append(torch.empty(nel, device=dev, dtype=dtype))
            shapes[5 * i:5 * i + 5] = [cout, cin, ks, stride, mode]
        self._shapes = shapes
        self._w = (C.c_void_p * self.n)(*[w.data_ptr() for w, _, _ in entries])
        self._p = (C.c_void_p * self.n)(*[b.data_ptr() for b in self.buffers])
        self._descs = torch.empty(max(1, self.n) * 4 * 64, device=dev, dtype=torch.uint8) if entries else None

    def pointers_current(self) -> bool:
        return all(w.data_ptr() == p for w, p in zip(self._keep, self._w))

    def refresh(self) -> None:
        if self.n:
            _launch(self._descs.device, _lib.load().hh_pack_conv_weights_batch_dt, ACT_DTYPES[self.dtype], self.n, self._w, self._p, self._shapes,
                    self._descs.data_ptr())


def _all_reduce_sums(sums: Tensor, group) -> None:
    import torch.distributed as dist
    dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group)  # RCCL on the GPU box; 2C doubles per layer


def sync_bn_train_forward(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, res: Tensor | None, relu: bool, group, world: int):
    """SyncBatchNorm forward (base/model.py:42-44): statistics over the pixels of ALL ranks of `group`.  Every rank must hold
    the same number of pixels (DistributedSampler with drop_last=True, datamodule.py:68-89).  -> (y, mean, invstd, count)"""
    lib = _lib.load()
    x = _nhwc(x)
    B, C, H, W = x.shape
    P = B * H * W
    y = torch.empty_like(x)
    mean, invstd, scratch = _bn_buffers(x)
    sums = torch.empty(2 * C, device=x.device, dtype=torch.float64)
    if res is not None:
        res = _nhwc(res)
    dt = _act(x, res)
    _launch(x.device, lib.hh_bn_train_stats_dt, dt, x.data_ptr(), P, C, sums.data_ptr(), scratch.data_ptr())
    _all_reduce_sums(sums, group)
    count = float(P) * world
    _launch(x.device, lib.hh_bn_train_normalize_dt, dt, x.data_ptr(), P, C, sums.data_ptr(), count, gamma.float().contiguous().data_ptr(),
            beta.float().contiguous().data_ptr(), eps, _ptr(res), int(relu), y.data_ptr(), mean.data_ptr(), invstd.data_ptr())
    return y, mean, invstd, count


def sync_bn_train_backward(x: Tensor, y: Tensor, dy: Tensor, mean: Tensor, invstd: Tensor, gamma: Tensor, relu: bool, want_dres: bool,
                           group, count: float):
    """-> (dx, dgamma, dbeta, dres or None); dgamma / dbeta are this rank's sums (DDP averages parameter gradients)."""
    lib = _lib.load()
    x, y, dy = _nhwc(x), _nhwc(y), _nhwc(dy)
    B, C, H, W = x.shape
    P = B * H * W
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    dgamma, dbeta, scratch = _bn_buffers(x)
    sums = torch.empty(2 * C, device=x.device, dtype=torch.float64)
    g = gamma.float().contiguous()
    dt = _act(x, y, dy)
    _launch(x.device, lib.hh_bn_train_backward_stats_dt, dt, x.data_ptr(), y.data_ptr(), dy.data_ptr(), P, C, mean.data_ptr(), invstd.data_ptr(),
            int(relu), sums.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), scratch.data_ptr())
    _all_reduce_sums(sums, group)
    _launch(x.device, lib.hh_bn_train_backward_apply_dt, dt, x.data_ptr(), y.data_ptr(), dy.data_ptr(), P, C, mean.data_ptr(), invstd.data_ptr(),
            g.data_ptr(), int(relu), sums.data_ptr(), count, dx.data_ptr(), _ptr(dres), scratch.data_ptr())
    return dx, dgamma, dbeta, dres


def conv2d_weight_grad(x: Tensor, dy: Tensor, ks: int, stride: int = 1, pad: tuple[int, int] | None = None) -> Tensor:
    """dL/dW [cout,cin,ks,ks] fp32 of y = conv(x, W) (padding (ks-1)/2) from the layer input x and dL/dy."""
    lib = _lib.load()
    x, dy = _nhwc(x), _nhwc(dy)
    B, cin, H, W = x.shape
    cout = dy.shape[1]
    dw = torch.empty((cout, cin, ks, ks), device=x.device, dtype=torch.float32)
    ws = torch.empty(lib.hh_conv2d_wgrad_workspace_bytes(B, H, W, cin, cout, ks, stride), device=x.device, dtype=torch.uint8)
    py_, px_ = pad if pad is not None else (-1, -1)
    _launch(x.device, lib.hh_conv2d_wgrad_dt, _act(x, dy), x.data_ptr(), dy.data_ptr(), B, H, W, cin, cout, ks, stride, py_, px_, dw.data_ptr(), ws.data_ptr())
    return dw


def fusion_sum(terms: list[Tensor], shifts: list[int], relu: bool = True) -> Tensor:
    """out = act(sum_j nearest_upsample(terms[j], 2 ** shifts[j])) (hh_fusion_sum_forward); terms[0] has the output resolution."""
    import ctypes as C
    lib = _lib.load()
    terms = [_nhwc(t) for t in terms]
    B, Cc, H, W = terms[0].shape
    out = torch.empty_like(terms[0])
    ptrs = (C.c_void_p * len(terms))(*[t.data_ptr() for t in terms])
    sh = (C.c_int * len(terms))(*shifts)
    _launch(out.device, lib.hh_fusion_sum_forward_dt, _act(*terms), ptrs, sh, len(terms), B, H, W, Cc, int(relu), out.data_ptr())
    return out


def fusion_sum_backward(dy: Tensor, out: Tensor, shifts: list[int], relu: bool = True) -> list[Tensor]:
    """-> the gradient of every term of fusion_sum (shift-0 terms share one tensor)."""
    import ctypes as C
    lib = _lib.load()
    dy, out = _nhwc(dy), _nhwc(out)
    B, Cc, H, W = dy.shape
    g = torch.empty_like(dy) if relu else dy
    ups = [(j, s) for j, s in enumerate(shifts) if s > 0]
    dups = [torch.empty((B, Cc, H >> s, W >> s), device=dy.device, dtype=dy.dtype).contiguous(memory_format=torch.channels_last) for _, s in ups]
    ptrs = (C.c_void_p * max(len(dups), 1))(*[t.data_ptr() for t in dups])
    sh = (C.c_int * max(len(dups), 1))(*[s for _, s in ups])
    _launch(dy.device, lib.hh_fusion_sum_backward_dt, _act(dy, out), dy.data_ptr(), out.data_ptr(), int(relu), B, H, W, Cc, g.data_ptr() if relu else None,
            ptrs, sh, len(dups))
    grads: list = [g] * len(shifts)
    for (j, _), d in zip(ups, dups):
        grads[j] = d
    return grads


# ------------------------------------------------------------------------------------------ the classifier's tail
def _f32(t: Tensor, what: str) -> Tensor:
    if not t.is_cuda:
        raise _lib.HHError(f"{what} must be a CUDA/HIP tensor: there is no CPU path")
    return t.detach().to(torch.float32).contiguous()


def global_avgpool(x: Tensor) -> Tensor:
    """[B,C,H,W] channels_last bf16 / fp16 -> fp32 [B,C]: the mean over the map (hh_global_avgpool)."""
    lib = _lib.load()
    x = _nhwc(x)
    B, C, H, W = x.shape
    out = torch.empty((B, C), device=x.device, dtype=torch.float32)
    _launch(x.device, lib.hh_global_avgpool_act, _act(x), x.data_ptr(), B, H * W, C, out.data_ptr())
    return out


def global_avgpool_backward(g: Tensor, H: int, W: int, dtype: torch.dtype) -> Tensor:
    """fp32 [B,C] -> [B,C,H,W] channels_last of `dtype`, every pixel g / (H W) (hh_global_avgpool_backward)."""
    lib = _lib.load()
    if dtype not in ACT_DTYPES:
        raise _lib.HHError(f"global_avgpool_backward: dtype must be torch.bfloat16 or torch.float16, not {dtype}")
    g = _f32(g, "the pooled gradient")
    B, C = g.shape
    dx = torch.empty((B, C, H, W), device=g.device, dtype=dtype, memory_format=torch.channels_last)
    _launch(g.device, lib.hh_global_avgpool_backward_act, ACT_DTYPES[dtype], g.data_ptr(), B, H * W, C, dx.data_ptr())
    return dx


def linear_forward(x: Tensor, w: Tensor, bias: Tensor) -> Tensor:
    """y = x w^T + bias, fp32 (hh_linear_forward)."""
    lib = _lib.load()
    x, w, bias = _f32(x, "x"), _f32(w, "w"), _f32(bias, "bias")
    (B, K), N = x.shape, w.shape[0]
    if w.shape != (N, K) or bias.shape != (N,):
        raise ValueError(f"linear_forward: x {tuple(x.shape)}, w {tuple(w.shape)}, bias {tuple(bias.shape)}")
    y = torch.empty((B, N), device=x.device, dtype=torch.float32)
    _launch(x.device, lib.hh_linear_forward, x.data_ptr(), w.data_ptr(), bias.data_ptr(), B, K, N, y.data_ptr())
    return y


def linear_backward(x: Tensor, w: Tensor, dy: Tensor, want=(True, True, True)):
    """-> (dx, dw, db) of y = x w^T + bias, fp32, each None where `want` is False (hh_linear_backward)."""
    lib = _lib.load()
    x, w, dy = _f32(x, "x"), _f32(w, "w"), _f32(dy, "dy")
    (B, K), N = x.shape, w.shape[0]
    if w.shape != (N, K) or dy.shape != (B, N):
        raise ValueError(f"linear_backward: x {tuple(x.shape)}, w {tuple(w.shape)}, dy {tuple(dy.shape)}")
    dx = torch.empty_like(x) if want[0] else None
    dw = torch.empty_like(w) if want[1] else None
    db = torch.empty(N, device=x.device, dtype=torch.float32) if want[2] else None
    _launch(x.device, lib.hh_linear_backward, x.data_ptr(), w.data_ptr(), dy.data_ptr(), B, K, N, _ptr(dx), _ptr(dw), _ptr(db))
    return dx, dw, db


def softmax_xent(logits: Tensor, targets: Tensor, want_grad: bool = True):
    """-> (result, dlogits or None).  result: int32 [4] on the device = hh_xent_result {loss (fp32 bits), top-1 hits, top-5 hits, flags};
    `read_xent_result` decodes a host copy.  Nothing here waits for the device."""
    lib = _lib.load()
    z = _f32(logits, "logits")
    B, N = z.shape
    t = targets.to(z.device, torch.int64).contiguous()
    if t.shape != (B,):
        raise ValueError(f"softmax_xent: logits {tuple(z.shape)}, targets {tuple(t.shape)}")
    result = torch.empty(4, device=z.device, dtype=torch.int32)
    dz = torch.empty_like(z) if want_grad else None
    _launch(z.device, lib.hh_softmax_xent, z.data_ptr(), t.data_ptr(), B, N, _ptr(dz), result.data_ptr())
    return result, dz


def read_xent_result(result: Tensor, B: int) -> dict:
    """One device -> host copy of an hh_xent_result -> {"loss", "top-1_error", "top-5_error"}; raises if the flag word says that a
    target was outside [0, N)."""
    r = result.cpu()
    if int(r[3]) & 1:
        raise IndexError("softmax cross-entropy: a target is outside [0, num_classes)")
    return {"loss": float(r[:1].view(torch.float32)), "top-1_error": 1.0 - int(r[1]) / B, "top-5_error": 1.0 - int(r[2]) / B}
