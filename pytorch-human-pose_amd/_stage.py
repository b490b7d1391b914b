"""How the batched descriptor calls move their inputs: `[descriptors | tables | uploaded frames | device-only outputs]` laid out in one
byte block (`Layout`), a pinned host copy of the uploaded prefix filled through numpy views and sent in ONE async copy (`Block`), a
`base` address plus offsets that may point at device tensors outside the block (`Block.off`, `Block.off_of`), frames that are uploaded
or read in place (`place_frames`, `fill_frames`), frames back through one pinned buffer (`frames_to_host`), and the two-slot pinned
ring of the input pipelines (`PinnedRing`).  torch is imported where it is needed: `align`, `per_frame` and `Layout` do without it,
and nothing here needs the library."""
from __future__ import annotations

import itertools
import math

import numpy as np


def align(n: int, a: int = 64) -> int:
    return (n + a - 1) // a * a


def per_frame(value, n: int) -> list:
    """One value, or one per frame (a list, a tuple or an array) -> a list."""
    return list(value) if isinstance(value, (list, tuple)) or np.ndim(value) else [value] * n


class Layout:
    """Sections appended to one byte block.  `end` is the block's size so far: a caller notes `upload = layout.end` where the
    device-only sections begin.  A caller with a layout of its own in front starts at its end."""

    def __init__(self, end: int = 0):
        self.end = int(end)

    def add(self, nbytes: int, align_to: int = 64) -> int:
        """-> the offset of a new section of `nbytes`, the next multiple of `align_to`."""
        at = align(self.end, align_to)
        self.end = at + int(nbytes)
        return at

    def pad(self, align_to: int = 64) -> int:
        """Round `end` up (the callers that align the end of a frame as well as its start) -> `end`."""
        self.end = align(self.end, align_to)
        return self.end


class Block:
    """The pinned host copy of the first `upload` bytes and the device block of `total` bytes.  `outside`: device tensors that
    descriptors point at though they lie elsewhere; the block keeps them alive."""

    def __init__(self, upload: int, total: int, device, outside=(), zero: bool = False):
        import torch
        self.pinned = torch.empty(upload, dtype=torch.uint8).pin_memory()
        self.bytes = self.pinned.numpy()
        if zero:
            self.bytes[:] = 0
        self.dev = torch.empty(total, dtype=torch.uint8, device=device)
        self.outside = list(outside)
        # offsets are counted from the lowest address involved, so that none is negative (the base itself is never dereferenced)
        self.base = min([self.dev.data_ptr()] + [t.data_ptr() for t in self.outside])
        self.rel = self.dev.data_ptr() - self.base

    def host(self, offset: int, count: int, dtype=np.uint8) -> np.ndarray:
        """`count` items of `dtype` of the pinned bytes from `offset` on."""
        return self.bytes[offset:offset + count * np.dtype(dtype).itemsize].view(dtype)

    def addr(self, offset: int) -> int:
        return self.dev.data_ptr() + offset

    def off(self, offset: int) -> int:
        """What a descriptor holds for the block's byte `offset`."""
        return self.rel + offset

    def off_of(self, tensor) -> int:
        """What a descriptor holds for a tensor of `outside`."""
        return tensor.data_ptr() - self.base

    def tensor(self, offset: int, shape):
        """A uint8 view of the device block."""
        return self.dev[offset:offset + math.prod(shape)].view(*shape)

    def upload(self) -> None:
        """The one async copy, on the current stream."""
        self.dev[:self.pinned.numel()].copy_(self.pinned, non_blocking=True)


def place_frames(layout: Layout, frames: list, device, pitched: bool = False) -> list:
    """One section per host frame (uint8 [h,w,3] array) -> per frame its offset, or None for a device tensor, which is read in place.
    `pitched`: a device frame may be a view with whole pixels and a row pitch (the JPEG encoder) instead of contiguous."""
    import torch
    places = []
    for f in frames:
        if isinstance(f, torch.Tensor):
            ok = f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3 and f.device == device
            if pitched and not (ok and f.stride(2) == 1 and f.stride(1) == 3 and f.stride(0) >= 3 * f.shape[1]):
                raise ValueError("a device frame must be a uint8 [h,w,3] tensor (or a view of one with whole pixels and a row pitch) on one device")
            if not pitched and not (ok and f.is_contiguous()):
                raise ValueError("a device frame must be a contiguous uint8 [h,w,3] tensor on one device")
            places.append(None)
        else:
            if not (isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] == 3):
                raise ValueError("a host frame must be a uint8 [h,w,3] array")
            places.append(layout.add(f.size))
    return places


def fill_frames(block: Block, frames: list, places: list) -> list:
    """The host frames copied into their sections -> per frame the `src` offset for its descriptor."""
    src = []
    for f, at in zip(frames, places):
        if at is None:
            src.append(block.off_of(f))
        else:
            np.copyto(block.host(at, f.size).reshape(f.shape), f)
            src.append(block.off(at))
    return src


def frames_to_host(frames: list, copy: bool = True) -> list:
    """Finished uint8 device frames back through ONE pinned buffer, behind one synchronize of the current stream -> numpy copies
    (`copy=False`: views of the pinned buffer, for a caller that turns them into something else at once)."""
    import torch
    if not frames:
        return []
    if any(f.dtype != torch.uint8 for f in frames):  # (the one buffer is bytes: another type would be converted, not carried)
        raise ValueError("frames_to_host: uint8 frames only")
    ends =list(itertools.accumulate(f.numel() for f in frames))
    host = torch.empty(ends[-1], dtype=torch.uint8, pin_memory=True)
    views = [host[end - f.numel():end].view(f.shape).copy_(f, non_blocking=True) for end, f in zip(ends, frames)]
    torch.cuda.current_stream(frames[0].device).synchronize()
    return [v.numpy().copy() if copy else v.numpy() for v in views]


class PinnedRing:
    """Two pinned staging buffers used in turn, each guarded by the event behind the copy that last read it."""

    def __init__(self):
        self.buffers = [None, None]
        self.free = [None, None]
        self.turn = 0

    def take(self, nbytes: int):
        """-> (the slot's index, its buffer of at least `nbytes`), once the copy that last read the buffer has finished."""
        import torch
        t = self.turn
        self.turn ^= 1
        if self.buffers[t] is None or self.buffers[t].numel() < nbytes:
            # (a larger buffer replaces the old one; the old one stays alive until its copy has run: torch keeps pinned blocks
            # that a non_blocking copy still reads)
            self.buffers[t] = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        elif self.free[t] is not None:
            self.free[t].synchronize()  # the copy that last read this buffer has finished
        return t, self.buffers[t]

    def release(self, turn: int, event) -> None:
        """`event`: recorded behind the copy that read slot `turn`'s buffer."""
        self.free[turn] = event
