"""Pose tracking across video frames: person ids that persist from frame to frame and One-Euro smoothed coordinates, computed on the
device behind hh_decode (hh_track_step; the rule is written at hh_track_step in include/hhrnet.h).  An extension: the reference has no
tracker.  Opt-in everywhere: without a PoseTracker every path runs as before.  There is no CPU fallback for `update_device`; the
`*_host` functions run the same code compiled for the host (tests, tools)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from .coco_eval import KPT_OKS_SIGMAS

MAX_TRACKS, MAX_K, MAX_PEOPLE, SOLVER_GUARD, POOL_FULL = (
    _lib.const("TRACK_" + k) for k in ("MAX_TRACKS", "MAX_K", "MAX_PEOPLE", "SOLVER_GUARD", "POOL_FULL"))
STATE_GLOBAL = 1  # hh_track_params.reserved bit 0: keep the state in global memory (tests)


Params = _lib.struct_ctype("hh_track_params")


def make_params(num_kpts=17, max_people=30, max_tracks=64, sigmas=KPT_OKS_SIGMAS, min_oks=0.3, max_age=30, joint_thr=0.05, min_joints=3,
                min_common=3, min_person_score=0.0, fps=30.0, min_cutoff=1.0, beta=0.007, d_cutoff=1.0, E=1, reserved=0) -> Params:
    """The parameter block; vars = (2 sigma)^2 formed here in float64.  Nothing is checked here: the entry points refuse what the rule
    cannot take."""
    p = Params()
    sig = np.asarray(sigmas, dtype=np.float64).reshape(-1)
    if len(sig) != num_kpts:
        raise ValueError(f"{len(sig)} sigmas for {num_kpts} keypoints")
    v = (sig * 2) ** 2
    for k in range(min(num_kpts, MAX_K)):
        p.vars[k] = v[k]
    p.fps, p.min_cutoff, p.beta, p.d_cutoff, p.min_oks = float(fps), float(min_cutoff), float(beta), float(d_cutoff), float(min_oks)
    p.joint_thr, p.min_person_score = float(joint_thr), float(min_person_score)
    p.K, p.E, p.max_people, p.max_tracks, p.max_age = int(num_kpts), int(E), int(max_people), int(max_tracks), int(max_age)
    p.min_joints, p.min_common, p.reserved = int(min_joints), int(min_common), int(reserved)
    return p


def state_bytes(num_kpts: int, max_tracks: int) -> int:
    n = _lib.load().hh_track_state_bytes(int(num_kpts), int(max_tracks))
    if n < 0:
        raise _lib.HHError(_lib.load().hh_last_error().decode())
    return n


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def step_host(params: Params, state: np.ndarray, joints, scores, num, flags=None, frames_per_stream: int = 1):
    """hh_track_step_host on numpy arrays; `state` (uint8, streams * state_bytes, 8-byte aligned) is updated in place.
    -> (ids [B,P], smooth [B,P,K,2], out_flags [B])."""
    joints, scores, num = _c(joints, np.float32), _c(scores, np.float32), _c(num, np.int32)
    flags = None if flags is None else _c(flags, np.int32)
    B, P, K = joints.shape[:3]
    ids, smooth, out = np.empty((B, P), np.int32), np.empty((B, P, K, 2), np.float32), np.empty(B, np.int32)
    F = int(frames_per_stream)
    _lib.check(_lib.load().hh_track_step_host(C.byref(params), state.ctypes.data, joints.ctypes.data, scores.ctypes.data, num.ctypes.data,
                                              None if flags is None else flags.ctypes.data, B // F if F else 0, F, ids.ctypes.data,
                                              smooth.ctypes.data, out.ctypes.data))
    return ids, smooth, out


def assign_host(sim, ids, min_oks: float) -> np.ndarray:
    """hh_track_assign_host: sim [n,T,P] float64, ids [n,T] int32 -> match [n,T]."""
    sim, ids = _c(sim, np.float64), _c(ids, np.int32)
    n, T, P = sim.shape
    match = np.empty((n, T), np.int32)
    _lib.check(_lib.load().hh_track_assign_host(sim.ctypes.data, ids.ctypes.data, n, T, P, float(min_oks), match.ctypes.data))
    return match


def assign_device(sim: torch.Tensor, ids: torch.Tensor, min_oks: float) -> torch.Tensor:
    """hh_track_assign on device tensors sim [n,T,P] float64, ids [n,T] int32, on the current stream -> match [n,T] int32."""
    n, T, P = sim.shape
    match = torch.empty((n, T), dtype=torch.int32, device=sim.device)
    _lib.launch(sim.device, _lib.load().hh_track_assign, sim.data_ptr(), ids.data_ptr(), n, T, P, float(min_oks), match.data_ptr())
    return match


class PoseTracker:
    """Ids and smoothing for `streams` independent video streams, state on the device.

    The arguments are the defaults of a parameter set, not measured optima: min_oks, max_age and the One-Euro constants (min_cutoff,
    beta, d_cutoff) have not been tuned on any clip.  `sigmas`: the per-keypoint OKS constants (COCO's by default).  A tracker is tied to
    one geometry: coordinates are model-input pixels, so frames of another model-input shape need `reset()` first."""

    def __init__(self, num_kpts=17, max_people=30, max_tracks=64, sigmas=KPT_OKS_SIGMAS, min_oks=0.3, max_age=30, joint_thr=0.05, min_joints=3,
                 min_common=3, min_person_score=0.0, fps=30.0, min_cutoff=1.0, beta=0.007, d_cutoff=1.0, streams=1, device="cuda:0"):
        self.params = make_params(num_kpts, max_people, max_tracks, sigmas, min_oks, max_age, joint_thr, min_joints, min_common,
                                  min_person_score, fps, min_cutoff, beta, d_cutoff)
        self.num_kpts, self.max_people, self.max_tracks, self.streams = int(num_kpts), int(max_people), int(max_tracks), int(streams)
        if self.streams < 1:
            raise ValueError("streams must be >= 1")
        self.device = torch.device(device)
        self._lib = _lib.load()
        self.state_bytes = state_bytes(num_kpts, max_tracks)
        # (an empty step_host call: the parameter block is refused here rather than at the first frame)
        z = np.zeros(8, np.float32)
        _lib.check(self._lib.hh_track_step_host(C.byref(self.params), z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, None, 0, 0,
                                                z.ctypes.data, z.ctypes.data, z.ctypes.data))
        self.state = torch.zeros(self.streams * self.state_bytes // 8, dtype=torch.int64, device=self.device)
        self.input_shape = None  # the model-input (h, w) the state's coordinates live in (set by InferenceKeypointsModel)

    def reset(self, stream: int | None = None) -> None:
        """Clear every stream's state, or that of one stream: ids start again at 1.  On the current torch stream."""
        if stream is None:
            first, n = 0, self.streams
            self.input_shape = None
        else:
            if not 0 <= stream < self.streams:
                raise IndexError(f"stream {stream} of {self.streams}")
            first, n = int(stream), 1
        _lib.launch(self.device, self._lib.hh_track_reset, self.state.data_ptr() + first * self.state_bytes, self.num_kpts, self.max_tracks, n)

    def bind_input_shape(self, shape) -> None:
        """The model-input shape of the frames fed so far; a different one raises (tracks live in model-input pixels)."""
        shape = tuple(int(v) for v in shape)
        if self.input_shape is None:
            self.input_shape = shape
        elif self.input_shape != shape:
            raise ValueError(f"PoseTracker: model-input shape changed from {self.input_shape} to {shape}; reset() the tracker first")

    def _check_inputs(self, joints, scores, num, flags, F):
        P, K = self.max_people, self.num_kpts
        if not (joints.is_cuda and joints.device == self.device):
            raise _lib.HHError("PoseTracker needs the decode's device tensors on its own device: there is no CPU path")
        if joints.dim() != 4 or tuple(joints.shape[1:3]) != (P, K) or joints.shape[3] < 3:
            raise ValueError(f"joints must be [B,{P},{K},3+E], got {tuple(joints.shape)}")
        B = joints.shape[0]
        if F < 1 or B != self.streams * F:
            raise ValueError(f"{B} frames for {self.streams} stream(s) of {F} frame(s)")
        for t, shape, dt in ((joints, None, torch.float32), (scores, (B, P), torch.float32), (num, (B,), torch.int32), (flags, (B,), torch.int32)):
            if t is None:
                continue
            if t.dtype != dt or not t.is_contiguous() or t.device != self.device or (shape is not None and tuple(t.shape) != shape):
                raise ValueError("PoseTracker: the inputs must be the contiguous tensors decode_batch_device returns")
        return B

    def update_device(self, joints, scores, num, flags=None, frames_per_stream: int = 1):
        """One hh_track_step on the current stream, no host synchronisation: the tensors of MPPEHeatmapParser.decode_batch_device for
        B = streams * frames_per_stream frames, stream-major (frame f of stream s is row s * frames_per_stream + f).
        -> (ids int32 [B,P], smooth float32 [B,P,K,2] in model-input pixels, out_flags int32 [B])."""
        F = int(frames_per_stream)
        B = self._check_inputs(joints, scores, num, flags, F)
        P, K = self.max_people, self.num_kpts
        self.params.E = int(joints.shape[3]) - 3
        ids = torch.empty((B, P), dtype=torch.int32, device=self.device)
        smooth = torch.empty((B, P, K, 2), dtype=torch.float32, device=self.device)
        out_flags = torch.empty((B,), dtype=torch.int32, device=self.device)
        _lib.launch(self.device, self._lib.hh_track_step, C.byref(self.params), self.state.data_ptr(), joints.data_ptr(), scores.data_ptr(),
                    num.data_ptr(), _lib.ptr(flags), self.streams, F, ids.data_ptr(), smooth.data_ptr(), out_flags.data_ptr())
        return ids, smooth, out_flags

    def similarity_device(self, joints, scores, num, flags=None) -> torch.Tensor:
        """hh_track_similarity: the [streams, max_tracks, max_people] float64 matrices of one frame per stream against the current
        state, which stays as it is."""
        self._check_inputs(joints, scores, num, flags, 1)
        self.params.E = int(joints.shape[3]) - 3
        sim = torch.empty((self.streams, self.max_tracks, self.max_people), dtype=torch.float64, device=self.device)
        _lib.launch(self.device, self._lib.hh_track_similarity, C.byref(self.params), self.state.data_ptr(), joints.data_ptr(), scores.data_ptr(),
                    num.data_ptr(), _lib.ptr(flags), self.streams, sim.data_ptr())
        return sim
