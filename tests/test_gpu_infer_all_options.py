"""`infer_images` with every option in one call: a tracker, a render that draws its ids, a score and JPEG inputs (bytes, indexed on the
device, and a host-indexed JpegImage) together, over three batches of which the last is short, so that pipeline slot 0 is used twice.
Each part of the combined call's results must equal, bit for bit, what the call with that option alone gives on the same list: a part
of the device -> host hand-over read under another part's name would show here."""
import importlib

import numpy as np
import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RENDER = dict(color_mode="track", alpha=0.65)


@pytest.fixture(scope="module")
def J(pkg):
    return importlib.import_module(PKG + ".keypoints.jpeg")


@pytest.fixture(scope="module")
def model(pkg):
    net = pkg.HigherHRNet(17, 32)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in pkg.synth.synth_passthrough_state_dict(shapes, 17, 0).items()})
    return pkg.InferenceKeypointsModel(net.to(DEV).eval(), det_thr=0.05, tag_thr=0.5, use_flip=False, input_size=128, device=DEV)


@pytest.fixture(scope="module")
def clip(J, model):
    """Five 96 x 128 frames of one clip, frame 1 as JPEG bytes and frame 3 as a host-indexed JpegImage, a plain run over that list, and
    annotations for frames 0, 1 and 3 made from that run's own predictions (every second person, shifted, some joints unlabelled)."""
    rs = np.random.RandomState(4)
    base = rs.randint(0, 255, (96, 128, 3)).astype(np.uint8)
    frames = [np.ascontiguousarray(np.roll(base, 2 * f, axis=1)) for f in range(5)]
    streams = {f: J.encode_jpeg_host(frames[f]) for f in (1, 3)}
    frames[1], frames[3] = streams[1], J.JpegImage(streams[3])
    plain = model.infer_images(frames, max_batch=2)
    annots = [None] * 5
    for i in (0, 1, 3):
        objs = []
        for p in range(0, len(plain[i].kpts_coords), 2):
            v = rs.randint(0, 3, 17)
            v[rs.randint(17)] = 2
            xy = np.where(v[:, None] > 0, np.round(plain[i].kpts_coords[p].astype(np.float64)) + rs.randint(-3, 4, (17, 2)), 0)
            x0, y0, x1, y1 = xy[v > 0, 0].min(), xy[v > 0, 1].min(), xy[v > 0, 0].max() + 20, xy[v > 0, 1].max() + 30
            objs.append({"image_id": i, "keypoints": np.concatenate([xy, v[:, None]], 1).astype(int).reshape(-1).tolist(),
                         "segmentation": [[x0, y0, x1, y0, x1, y1, x0, y1]]})
        annots[i] = objs
    return frames, streams, plain, annots


def test_every_option_at_once_equals_each_option_alone(pkg, J, model, clip):
    tk = importlib.import_module(PKG + ".keypoints.tracking")
    frames, _, plain, annots = clip
    tracked = model.infer_images(frames, max_batch=2, tracker=tk.PoseTracker(device=DEV), render=RENDER)
    scored = model.infer_images(frames, annots=annots, max_batch=2, score="oks")
    both = model.infer_images(frames, annots=annots, max_batch=2, tracker=tk.PoseTracker(device=DEV), render=RENDER, score="oks")
    people = [len(r.kpts_coords) for r in plain]
    print("people:", people, "ids issued:", max(int(r.track_ids.max(initial=0)) for r in both), "oks:", [r.oks for r in both])
    assert sum(people) > 0 and any(a for a in annots if a) and any((r.track_ids != 0).any() for r in tracked)
    for i, (p, t, s, c) in enumerate(zip(plain, tracked, scored, both)):
        for f in ("kpts_coords", "kpts_scores", "kpts_tags"):
            assert np.array_equal(getattr(c, f), getattr(p, f)), (i, f)
        assert c.track_ids.dtype == np.int32 and c.track_ids.shape == (people[i],) and np.array_equal(c.track_ids, t.track_ids), i
        assert c.kpts_coords_smooth.shape == p.kpts_coords.shape and c.kpts_coords_smooth.tobytes() == t.kpts_coords_smooth.tobytes(), i
        assert c.rendered.shape == (96, 128, 3) and np.array_equal(c.rendered, t.rendered), i
        if annots[i] is None:
            assert c.oks is None and s.oks is None and c.target_matches is None
            continue
        assert c.oks == s.oks and c.object_oks.shape == (len(annots[i]),), i
        for f in ("object_oks", "kpt_oks", "target_matches"):
            assert getattr(c, f).tobytes() == getattr(s, f).tobytes(), (i, f)


def test_a_cut_stream_raises_when_its_batch_is_collected(pkg, J, model, clip):
    """Frame 3 lies in the second of three batches, which is collected behind the enqueue of the third: all three decodes have been
    enqueued when the error is raised."""
    tk = importlib.import_module(PKG + ".keypoints.tracking")
    frames, streams, _, annots = clip
    cut = list(frames)
    cut[3] = J.JpegImage(streams[3][:J.jpeg_info(streams[3]).scan_end - 10], index=J.build_jpeg_index(streams[3]))
    decode, calls = model._parser.decode_batch_device, []

    def counting(*args, **kwargs):
        calls.append(len(calls))
        return decode(*args, **kwargs)
    model._parser.decode_batch_device = counting
    try:
        with pytest.raises(pkg._lib.HHError, match=r"infer_images: image 3: its JPEG stream cannot be decoded: status 3 \(bytes exhausted\)"):
            model.infer_images(cut, annots=annots, max_batch=2, tracker=tk.PoseTracker(device=DEV), render=RENDER, score="oks")
    finally:
        del model._parser.decode_batch_device
    assert len(calls) == 3
    torch.cuda.synchronize()
