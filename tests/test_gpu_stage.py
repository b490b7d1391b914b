"""-m gpu: the parts of `_stage.py` that touch the device (`Block`, `frames_to_host`, `PinnedRing`).  No project kernel is launched."""
import importlib

import numpy as np
import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def st():
    return importlib.import_module(PKG + "._stage")


def test_block_offsets_and_upload(st):
    rng = np.random.default_rng(1)
    before = torch.full((3, 4, 3), 7, dtype=torch.uint8, device=DEV)
    dummy = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)  # (keeps the two device frames and the block apart)
    after = torch.full((2, 9, 3), 9, dtype=torch.uint8, device=DEV)
    host_frame = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    frames = [before, host_frame, after]
    lay = st.Layout()
    desc_at = lay.add(48 * 3)
    places = st.place_frames(lay, frames, DEV)
    assert places[0] is None and places[2] is None and places[1] == 192
    upload = lay.pad()
    out_at = lay.add(1000)
    blk = st.Block(upload, lay.pad(), DEV, [before, after])
    assert blk.pinned.is_pinned() and blk.pinned.numel() == upload and blk.dev.numel() == lay.end
    assert blk.base == min(blk.dev.data_ptr(), before.data_ptr(), after.data_ptr()) and blk.rel == blk.dev.data_ptr() - blk.base
    for at in (desc_at, places[1], out_at):
        assert blk.off(at) >= 0 and blk.base + blk.off(at) == blk.addr(at) == blk.dev.data_ptr() + at
    for t in (before, after):
        assert blk.off_of(t) >= 0 and blk.base + blk.off_of(t) == t.data_ptr()
    assert blk.tensor(out_at, (10, 100)).data_ptr() == blk.addr(out_at)

    blk.tensor(upload, (lay.end - upload,)).fill_(0xA5)
    blk.host(desc_at, 3 * 6, np.int64)[:] = np.arange(18)
    src = st.fill_frames(blk, frames, places)
    assert src == [blk.off_of(before), blk.off(places[1]), blk.off_of(after)]
    blk.upload()
    torch.cuda.current_stream(DEV).synchronize()
    assert np.array_equal(blk.tensor(places[1], host_frame.shape).cpu().numpy(), host_frame)
    assert np.array_equal(blk.tensor(desc_at, (144,)).cpu().numpy().view(np.int64), np.arange(18))
    assert bool((blk.tensor(upload, (lay.end - upload,)) == 0xA5).all())  # nothing past the uploaded prefix is written
    assert bool((before == 7).all()) and bool((after == 9).all())
    del dummy

    zeroed = st.Block(100, 200, DEV, zero=True)
    assert not zeroed.bytes.any() and zeroed.base == zeroed.dev.data_ptr() and zeroed.rel == 0


def test_frames_to_host(st):
    g = torch.Generator(device="cpu").manual_seed(2)
    frames = [torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).to(DEV) for shape in [(1, 1, 3), (5, 7, 3), (64, 37, 3)]]
    got = st.frames_to_host(frames)
    assert len(got) == 3
    for a, f in zip(got, frames):
        assert a.dtype == np.uint8 and a.shape == tuple(f.shape) and a.flags.owndata and np.array_equal(a, f.cpu().numpy())
    for a, f in zip(st.frames_to_host(frames, copy=False), frames):  # views of the one pinned buffer
        assert not a.flags.owndata and np.array_equal(a, f.cpu().numpy())
    assert st.frames_to_host([]) == []


def test_pinned_ring(st):
    ring = st.PinnedRing()
    t0, b0 = ring.take(100)
    t1, b1 = ring.take(100)
    assert t0 != t1 and b0.data_ptr() != b1.data_ptr() and b0.is_pinned() and b1.is_pinned() and b0.numel() >= 100
    dst = torch.empty(100, dtype=torch.uint8, device=DEV)
    dst.copy_(b0, non_blocking=True)
    event = torch.cuda.Event()
    event.record()
    ring.release(t0, event)
    t2, b2 = ring.take(100)
    assert t2 == t0 and b2.data_ptr() == b0.data_ptr() and event.query()  # (take waited for the copy that read the buffer)
    t3, b3 = ring.take(5000)  # slot t1 grows; slot t0 keeps its buffer
    assert t3 == t1 and b3.numel() >= 5000 and b3.data_ptr() != b1.data_ptr()
    t4, b4 = ring.take(50)
    assert t4 == t0 and b4.data_ptr() == b0.data_ptr()
