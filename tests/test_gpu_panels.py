"""-m gpu: the heatmap panels (hh_heatmap_panels_u8), the un-normalise (hh_unnormalize_u8) and the fx / fy resize (hh_resize_u8_scaled)
against their numpy restatements (tests/panels_ref.py), bit-identical on every byte, and the Python interface built on them
(plot_heatmaps, InferenceKeypointsResult.plot, KeypointsResult.plot).  The lattice is tests/panels_helpers.py: all shapes are tiny."""
import importlib

import numpy as np
import pytest
import torch

import cv_resize
import panels_ref as pr
import render_ref as rr
from conftest import PKG
from panels_helpers import image_of, lattice
from render_helpers import vis  # noqa: F401
from test_gpu_render import model  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _placed_dev(vis, grids, H, W):
    placed, Hc, Wc = vis.figure_layout(grids, H, W)
    return [(k, _dev(a), _dev(b), f, oy, ox) for k, a, b, f, oy, ox in placed], placed, Hc, Wc


@pytest.fixture(scope="module")
def cases():
    """The lattice with its references, computed once."""
    lut = pr.jet_lut()
    return [(name, img, grids, pr.figure(img, grids, lut)) for name, img, grids in lattice()]


def test_lattice_device_equals_reference_equals_host(vis, cases):
    for name, img, grids, ref in cases:
        on_dev, placed, Hc, Wc = _placed_dev(vis, grids, *img.shape[:2])
        got = vis.to_host(vis.panels_device(_dev(img), on_dev, Hc, Wc))
        assert got.shape == ref.shape and np.array_equal(got, ref), (name, int((got != ref).sum()))
        assert np.array_equal(vis.panels_host(img, placed, Hc, Wc), got), name


def test_no_stale_state(vis, cases):
    """The same figure twice in a row, then a figure of another size, then the first again: identical bytes every time (nothing of
    the reduction is carried from call to call)."""
    pick = [c for c in cases if c[0] in ("mixed_8x12_K17_r2", "kind3_flags2", "mixed_5x7_K3_r2")]
    assert len(pick) == 3

    def run(c):
        on_dev, _, Hc, Wc = _placed_dev(vis, c[2], *c[1].shape[:2])
        return vis.to_host(vis.panels_device(_dev(c[1]), on_dev, Hc, Wc))

    for c in (pick[0], pick[0], pick[1], pick[0], pick[2], pick[1], pick[0]):
        assert np.array_equal(run(c), c[3]), c[0]


@pytest.mark.parametrize("offset,slack", [(0, 0), (1, 0), (2, 3), (3, 7)])
def test_canvas_fully_written_at_any_address_and_pitch(vis, cases, offset, slack):
    """The destination starts as 0xA5 everywhere: the cells, the padding and the unused cell are all written, the bytes between a row's
    end and the pitch and around the canvas are not.  Canvas addresses 0..3 modulo 4, pitches that are no multiple of 4."""
    for name, img, grids, ref in [c for c in cases if c[0] in ("mixed_5x7_K3_r2", "mixed_16x16_K3_r1", "kind0_flags0")]:
        on_dev, _, Hc, Wc = _placed_dev(vis, grids, *img.shape[:2])
        pitch = Wc * 3 + slack
        buf = torch.full((offset + Hc * pitch + 8,), 0xA5, dtype=torch.uint8, device=DEV)
        vis.panels_device(_dev(img), on_dev, Hc, Wc, canvas=buf[offset:offset + Hc * pitch], pitch=pitch)
        torch.cuda.synchronize()
        flat = buf.cpu().numpy()
        rows = flat[offset:offset + Hc * pitch].reshape(Hc, pitch)
        assert np.array_equal(rows[:, :Wc * 3].reshape(Hc, Wc, 3), ref), name
        assert (rows[:, Wc * 3:] == 0xA5).all() and (flat[:offset] == 0xA5).all() and (flat[offset + Hc * pitch:] == 0xA5).all(), name


def test_unnormalize_u8(vis):
    """Every byte value normalised as the model input is, then values that un-normalise below 0 and above 255."""
    H, W = 20, 28
    raw = np.resize(np.arange(256, dtype=np.uint8), (H, W, 3)).copy()
    raw[..., 1] = raw[..., 1][::-1]
    x = ((raw.astype(np.float32) / np.float32(255) - pr.MEAN.astype(np.float32)) / pr.STD.astype(np.float32)).astype(np.float32).transpose(2, 0, 1).copy()
    x[:, 0, :8] = [-2.5, -2.2, -2.118, 2.64, 2.7, 3.5, 40.0, -40.0]
    x[:, 1, :4] = [np.nan, np.inf, -np.inf, 1e30]
    want = pr.inverse_transform(x)
    got = vis.to_host(vis.unnormalize_device(_dev(x)))
    assert got.shape == (H, W, 3) and np.array_equal(got, want), int((got != want).sum())
    assert (np.abs(got[2:].astype(int) - raw[2:].astype(int)) <= 1).all() and (got[2:] <= raw[2:]).all()  # the truncation: never above, at most one below


def test_resize_u8_scaled(vis):
    src = image_of(79, 111, 3)
    for fx, fy in ((0.6, 0.6), (0.4, 0.4), (0.6, 0.4), (0.35, 1.3)):
        want = pr.resize_scaled(src, fx, fy)
        got = vis.to_host(vis.resize_scaled_device(_dev(src), fx, fy))
        assert got.shape == want.shape and np.array_equal(got, want), (fx, fy)
    # cvRound lands on a half: 5 * 0.5 = 2.5 -> 2, 7 * 0.5 = 3.5 -> 4
    for h, w in ((5, 7), (7, 5), (9, 33)):
        s = image_of(h, w, 2)
        got = vis.to_host(vis.resize_scaled_device(_dev(s), 0.5, 0.5))
        assert got.shape == (pr.scaled_size(h, 0.5), pr.scaled_size(w, 0.5), 3) and np.array_equal(got, pr.resize_scaled(s, 0.5, 0.5)), (h, w)
    assert vis.scaled_size(5, 0.5) == 2 and vis.scaled_size(7, 0.5) == 4
    # fx = W / w exactly: equal to hh_resize_u8, on the taps and on the 2 x 2 mean
    for (h, w), f in (((64, 48), 0.5), ((64, 48), 0.25), ((37, 48), 2.0), ((16, 24), 1.5)):
        s = _dev(image_of(h, w, 1))
        a = vis.to_host(vis.resize_scaled_device(s, f, f))
        b = vis.to_host(vis.resize_device(s, int(w * f), int(h * f)))
        assert np.array_equal(a, b) and np.array_equal(a, cv_resize.resize(image_of(h, w, 1), (int(w * f), int(h * f)))), (h, w, f)


def test_plot_heatmaps(pkg, vis, cases):
    """plot_heatmaps returns the cells of the corresponding figure, from numpy arrays and from device tensors."""
    lut = pr.jet_lut()
    name, img, grids, ref = next(c for c in cases if c[0] == "kind0_flags3")
    hms = np.stack([m[1] for m in grids[0][0]])
    for clip, minmax in ((False, False), (True, False), (False, True), (True, True)):
        want = [pr.cell(img, hm, (pr.CLIP if clip else 0) | (pr.MINMAX if minmax else 0), lut) for hm in hms]
        before = hms.copy()
        for got in (pkg.keypoints.plot_heatmaps(img, hms, clip_0_1=clip, minmax=minmax), pkg.keypoints.plot_heatmaps(_dev(img), _dev(hms), clip, minmax)):
            assert len(got) == len(want) and all(g.dtype == np.uint8 and np.array_equal(g, w) for g, w in zip(got, want)), (clip, minmax)
        assert np.array_equal(hms, before, equal_nan=True)
    # the same cells as the figure's
    _, _, at = pr.grid_layout(len(hms), 2, img.shape[0], img.shape[1], 5)
    got = pkg.keypoints.plot_heatmaps(img, hms, True, True)
    for (y, x), g in zip(at, got):
        assert np.array_equal(ref[y:y + img.shape[0], x:x + img.shape[1]], g)


def _cpu(t):
    return t.detach().float().cpu().numpy()


def test_end_to_end_inference_plot(model, vis):
    image = np.random.RandomState(5).randint(0, 255, (150, 220, 3)).astype(np.uint8)
    res = model(image, None)
    plots = res.plot()
    assert set(plots) == {"connections", "heatmaps"}
    palette = importlib.import_module(PKG + ".keypoints.visualization").DEFAULT_PALETTE
    assert np.array_equal(plots["connections"], rr.render(res.raw_image, res.kpts_coords, res.kpts_scores, res.limbs, res.det_thr, "person", 0.8, palette))
    assert np.array_equal(plots["connections"], res.plot_connections())
    hm_q, hm_h, tags = _cpu(res._stage_hms[0][0]), _cpu(res._stage_hms[1][0]), _cpu(res._tags[0][0])
    x = _cpu(res.model_input_image)
    assert x.shape[0] == 3 and hm_q.shape[0] == 17 and (4 * hm_q.shape[1], 4 * hm_q.shape[2]) == x.shape[1:]
    want = pr.inference_figure(pr.inverse_transform(x), hm_q, hm_h, tags, pr.jet_lut())
    got = plots["heatmaps"]
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    # the properties are what they were
    assert res.kpts_heatmaps.shape == (17,) + x.shape[1:] and res.tags_heatmaps.shape == (17,) + x.shape[1:]


def test_end_to_end_validation_plot(pkg, model, vis):
    image = np.random.RandomState(6).randint(0, 255, (128, 128, 3)).astype(np.uint8)
    res = model(image, None)
    x = res.model_input_image
    vres = pkg.keypoints.KeypointsResult(x.cpu(), [h[:1] for h in res._stage_hms], res._tags[0][:1], res.limbs, 20, 0.1, 1.0)
    vres.set_preds()
    got = vres.plot()
    assert set(got) == {"heatmaps"}
    got = got["heatmaps"]
    img = pr.inverse_transform(_cpu(x))
    palette = importlib.import_module(PKG + ".keypoints.visualization").DEFAULT_PALETTE
    conn = rr.render(img, vres.kpts_coords, vres.kpts_scores, vres.limbs, vres.det_thr, "person", 0.8, palette)
    want = pr.validation_figure(img, conn, _cpu(res._stage_hms[0][0]), _cpu(res._stage_hms[1][0]), _cpu(res._tags[0][0]), pr.jet_lut())
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())


def test_bad_arguments_launch_nothing(pkg, vis):
    """A refused call returns an error before any launch: the 0xA5 canvas is untouched."""
    lib = pkg._lib.load()
    H, W = 20, 28
    img, m, q = _dev(image_of(H, W, 0)), torch.zeros((H, W), device=DEV), torch.zeros((5, 7), device=DEV)
    lut = _dev(pr.jet_lut())
    canvas = torch.full((H + 10, W + 10, 3), 0xA5, dtype=torch.uint8, device=DEV)
    scratch = torch.zeros(64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(rows, lut_ptr=lut.data_ptr(), Hc=H + 10, Wc=W + 10, pitch=(W + 10) * 3):
        table = np.zeros(len(rows), vis.PANEL)
        for i, (kind, src, flags, oy, ox) in enumerate(rows):
            table[i] = (src.data_ptr(), 0, src.shape[0], src.shape[1], kind, flags, oy, ox)
        dev = _dev(table.view(np.uint8))
        return lib.hh_heatmap_panels_u8(dev.data_ptr(), table.ctypes.data, len(rows), img.data_ptr(), H, W, lut_ptr, canvas.data_ptr(), Hc, Wc, pitch,
                                        scratch.data_ptr(), stream)

    good = [(pr.DIRECT, m, 0, 5, 5)]
    bad = [dict(rows=good, lut_ptr=None),                       # a null colour table
           dict(rows=[(4, m, 0, 5, 5)]), dict(rows=[(-1, m, 0, 5, 5)]),   # a kind out of range
           dict(rows=[(pr.DIRECT, m, 0, 11, 5)]), dict(rows=[(pr.DIRECT, m, 0, 5, -1)]), dict(rows=good, Hc=H + 4),   # a cell outside the canvas
           dict(rows=[(pr.DIRECT, q, 0, 5, 5)]),                 # DIRECT with a size mismatch
           dict(rows=[(pr.NESTED, m, 0, 5, 5)]), dict(rows=[(pr.AVERAGE, q, 0, 5, 5)]),   # not a quarter; AVERAGE without its half-resolution map
           dict(rows=[(pr.DIRECT, m, 8, 5, 5)]), dict(rows=good, pitch=(W + 10) * 3 - 1), dict(rows=[])]
    for kw in bad:
        assert call(**kw) == 1 and lib.hh_last_error(), kw
    torch.cuda.synchronize()
    assert (canvas.cpu().numpy() == 0xA5).all()
    assert call(good) == 0
    torch.cuda.synchronize()
    out = canvas.cpu().numpy()
    assert (out[:5] == 0).all() and (out[5:5 + H, 5:5 + W] != 0xA5).any()
    with pytest.raises(pkg._lib.HHError):
        vis.resize_scaled_device(img, 0.0, 0.5)
    src = _dev(image_of(5, 7, 0))
    dst = torch.empty((3, 4, 3), dtype=torch.uint8, device=DEV)
    assert lib.hh_resize_u8_scaled(src.data_ptr(), 5, 7, 3, 0.5, 0.5, dst.data_ptr(), 3, 4, stream) == 1   # cvRound(2.5) is 2, not 3
