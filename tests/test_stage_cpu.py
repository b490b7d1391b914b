"""`_stage.py` without a GPU: `Layout` against the byte layouts the batched calls had before they shared it (each formula written out
here, none computed through `Layout`), its invariants, the refusals of `place_frames`, and `per_frame`."""
import importlib

import numpy as np
import pytest

from conftest import PKG

FRAMES = [(1, 1), (5, 7), (64, 37)]
BATCHES = [[f] for f in FRAMES] + [FRAMES]  # n = 1 and n = 3


@pytest.fixture(scope="module")
def st():
    return importlib.import_module(PKG + "._stage")


def a64(x):
    return (x + 63) // 64 * 64


def a16(x):
    return (x + 15) // 16 * 16


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("table_len", [0, 7])
def test_render_layout(pkg, st, batch, table_len):
    """[descriptors | table | uploaded frames | outputs]: D * n, then P * total at align64, then every frame with start and end at align64."""
    D, P = pkg._lib.struct_dtype("hh_render_desc").itemsize, pkg._lib.struct_dtype("hh_render_prim").itemsize
    n, total = len(batch), table_len * len(batch)
    sizes = [h * w * 3 for h, w in batch]
    prim_at = a64(D * n)
    at = a64(prim_at + P * total)
    src_at = []
    for s in sizes:
        src_at.append(at)
        at = a64(at + s)
    upload = at
    out_at = []
    for s in sizes:
        out_at.append(at)
        at = a64(at + s)

    lay = st.Layout()
    assert lay.add(D * n) == 0
    assert lay.add(P * total) == prim_at
    assert [lay.add(s) for s in sizes] == src_at
    assert lay.pad() == upload == lay.end
    assert [lay.add(s) for s in sizes] == out_at
    assert lay.pad() == at


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("table_len", [0, 7])
def test_decode_layout(pkg, st, batch, table_len):
    """[descriptors | streams and tables | statuses | pixels]: align16(desc * n), the streams unpadded back to back (each a multiple of
    16 as JpegImage.staged_bytes gives it), align16 statuses of 8 n bytes, every pixel slot at align16."""
    desc, seg = pkg._lib.struct_dtype("hh_jpeg_dec_desc").itemsize, pkg._lib.struct_dtype("hh_jpeg_segment").itemsize
    n = len(batch)
    staged = [a16(h * w + 5) + a16(seg * table_len) for h, w in batch]
    at = a16(desc * n)
    places = []
    for s in staged:
        places.append(at)
        at += s
    upload = at
    status_at = a16(at)
    at = status_at + 4 * n * 2
    dst_at = []
    for h, w in batch:
        at = a16(at)
        dst_at.append(at)
        at += h * w * 3

    lay = st.Layout()
    assert lay.add(desc * n, 16) == 0
    assert [lay.add(s, 16) for s in staged] == places
    assert lay.end == upload
    assert lay.add(8 * n, 16) == status_at
    assert [lay.add(h * w * 3, 16) for h, w in batch] == dst_at
    assert lay.end == at


def test_layout_invariants(st):
    rng = np.random.default_rng(0)
    lay, end = st.Layout(), 0
    for _ in range(200):
        nbytes, a = int(rng.integers(0, 300)), int(rng.choice([1, 4, 8, 16, 64]))
        at = lay.add(nbytes, a)
        assert at % a == 0 and at >= end          # aligned, and behind everything added before
        assert lay.end == at + nbytes >= end      # monotonic
        end = lay.end
        if rng.integers(0, 4) == 0:
            assert lay.pad(a) == lay.end >= end and lay.end % a == 0 and lay.end - end < a
            end = lay.end
    assert st.align(0) == 0 and st.align(1) == 64 and st.align(64) == 64 and st.align(65) == 128 and st.align(17, 16) == 32


@pytest.mark.parametrize("frame", [np.zeros((5, 7, 3), np.float32), np.zeros((5, 7, 4), np.uint8), np.zeros((5, 7), np.uint8),
                                   np.zeros((5, 7, 3), np.uint8).tolist()], ids=["float", "hw4", "2d", "list"])
@pytest.mark.parametrize("pitched", [False, True])
def test_place_frames_refuses(st, frame, pitched):
    lay = st.Layout()
    with pytest.raises(ValueError, match=r"a host frame must be a uint8 \[h,w,3\] array"):
        st.place_frames(lay, [np.zeros((2, 2, 3), np.uint8), frame], None, pitched)


def test_place_frames_refuses_device_frames(st):
    """The two device-frame rules, on CPU tensors (the rules read dtype, shape, strides and device only)."""
    import torch
    cpu = torch.device("cpu")
    plain, pitch = r"a device frame must be a contiguous uint8 \[h,w,3\] tensor on one device", r"whole pixels and a row pitch"
    wide = torch.zeros((5, 9, 3), dtype=torch.uint8)
    good, columns = torch.zeros((5, 7, 3), dtype=torch.uint8), wide[:, 1:8]  # columns: rows 27 bytes apart, 21 used
    for pitched in (False, True):
        lay = st.Layout()
        assert st.place_frames(lay, [good], cpu, pitched) == [None] and lay.end == 0  # read in place: no section
    assert st.place_frames(st.Layout(), [columns], cpu, pitched=True) == [None]
    with pytest.raises(ValueError, match=plain):
        st.place_frames(st.Layout(), [columns], cpu)  # a row pitch is the encoder's alone
    bad = {"float": good.float(), "hw4": torch.zeros((5, 7, 4), dtype=torch.uint8), "2d": good[:, :, 0], "meta device": good.to("meta"),
           "every other pixel": wide[:, ::2], "channel stride": torch.zeros((5, 7, 6), dtype=torch.uint8)[:, :, ::2],
           "rows overlap": good.as_strided((5, 7, 3), (3, 3, 1))}
    for name, f in bad.items():
        with pytest.raises(ValueError, match=plain):
            st.place_frames(st.Layout(), [good, f], cpu)
        with pytest.raises(ValueError, match=pitch):
            st.place_frames(st.Layout(), [good, f], cpu, pitched=True)


def test_frames_to_host_refuses_another_dtype(st):
    import torch
    with pytest.raises(ValueError, match="uint8 frames only"):
        st.frames_to_host([torch.zeros((2, 2, 3), dtype=torch.uint8), torch.zeros((2, 2, 3))])  # (refused before any allocation)


def test_text_tile_list_does_not_read_the_frame_offsets(pkg):
    """`stage_put_txt` sizes and fills its tile list before the block exists, with both offsets 0, and writes the offsets counted from
    the block's base afterwards: hh_text_tiles must give the same list whatever the (equal, non-negative) offsets are."""
    import ctypes as C
    tx = importlib.import_module(PKG + ".keypoints.text")
    lib, atlas_len = pkg._lib.load(), len(tx.font().coverage)
    tables = [tx.layout_put_txt(70, 200, ["first line", "second"]), tx.video_table(150, 300, ["0 / 3", "Latency [ms]: "])]
    prims = np.concatenate(tables)

    def tiles(offsets):
        descs = np.zeros(2, tx.DESC)
        descs[0] = (offsets[0], offsets[0], 70, 200, 0, len(tables[0]), 0.0, 0.0, 0, 0)
        descs[1] = (offsets[1], offsets[1], 150, 300, len(tables[0]), len(tables[1]), 0.0, 0.0, 0, 0)
        count = C.c_longlong(0)
        pkg._lib.check(lib.hh_text_tiles(descs.ctypes.data, prims.ctypes.data, len(prims), 2, atlas_len, None, 0, C.byref(count)))
        listed = np.zeros(2 * count.value, np.int32)
        pkg._lib.check(lib.hh_text_tiles(descs.ctypes.data, prims.ctypes.data, len(prims), 2, atlas_len, listed.ctypes.data, count.value, C.byref(count)))
        pkg._lib.check(lib.hh_text_check(descs.ctypes.data, prims.ctypes.data, len(prims), 2, atlas_len, listed.ctypes.data, count.value))
        return listed

    zero = tiles((0, 0))
    assert len(zero) > 0
    assert np.array_equal(zero, tiles((1 << 33, 12345))) and np.array_equal(zero, tiles((7, (1 << 40) + 1)))


def test_place_frames_adds_one_section_per_host_frame(st):
    lay = st.Layout()
    lay.add(10)
    frames = [np.zeros((h, w, 3), np.uint8) for h, w in FRAMES]
    assert st.place_frames(lay, frames, None) == [64, 128, 128 + a64(5 * 7 * 3)]
    assert lay.end == 128 + a64(5 * 7 * 3) + 64 * 37 * 3


def test_per_frame(st):
    assert st.per_frame(0.4, 3) == [0.4, 0.4, 0.4]
    assert st.per_frame("420", 2) == ["420", "420"]
    assert st.per_frame(None, 2) == [None, None]
    assert st.per_frame([1, 2, 3], 3) == [1, 2, 3]
    assert st.per_frame((True, False), 2) == [True, False]
    assert st.per_frame(np.array([0.25, 0.5]), 2) == [0.25, 0.5]
