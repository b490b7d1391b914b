"""Pose tracking on the GPU (hh_track_step, hh_track_similarity, hh_track_assign; keypoints/tracking.py) against the host form and the
numpy restatement of tests/track_ref.py, on the clips whose margin tests/test_track_cpu.py asserts, and end to end through
InferenceKeypointsModel.video_frame / infer_images at 128 x 128 on synthetic weights."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import track_ref as tr
from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = ("kpts_coords", "kpts_scores", "kpts_tags", "obj_scores")


@pytest.fixture(scope="module")
def tk():
    return importlib.import_module(PKG + ".keypoints.tracking")


def tracker_for(tk, case, S=None, reserved=0):
    t = tk.PoseTracker(case["K"], case["P"], case["T"], tr.sigmas_for(case["K"]), streams=case["S"] if S is None else S, device=DEV,
                       **dict(tr.DEFAULTS, **case.get("kw", {})))
    t.params.reserved = reserved
    return t


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_run(tk, case, clip=None, S=None, chunks=None, reserved=0):
    """The clip through hh_track_step in `chunks` (default: one call) -> (ids, smooth, flags, state) as numpy arrays."""
    clip = tr.case_clip(case)[0] if clip is None else clip
    S = case["S"] if S is None else S
    t = tracker_for(tk, case, S, reserved)
    F = len(clip[2]) // S
    outs, at = [], 0
    for n in chunks or [F]:
        sel = np.concatenate([np.arange(s * F + at, s * F + at + n) for s in range(S)])
        o = t.update_device(*(dev(p[sel]) for p in clip), frames_per_stream=n)
        outs.append([a.cpu().numpy().reshape((S, n) + tuple(a.shape[1:])) for a in o])
        at += n
    return [np.concatenate([o[i] for o in outs], 1).reshape((S * F,) + outs[0][i].shape[2:]) for i in range(3)] + [t.state.cpu().numpy()]


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("case", tr.GPU_CASES, ids=lambda c: c["name"])
def test_step_equals_host_form(tk, case):
    clip, refs = tr.case_clip(case)
    got = dev_run(tk, case)
    want = tr.host_run(tk, clip, case["K"], case["P"], case["T"], case["S"], **case.get("kw", {}))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    assert got[1].tobytes() == want[1].tobytes()
    assert got[3].tobytes() == want[3].tobytes()  # the state: nothing in it comes from exp()
    F = len(clip[2]) // case["S"]
    for s, (rid, rsm, rfl, _) in enumerate(refs):  # and the restatement
        assert np.array_equal(got[0][s * F:(s + 1) * F], rid) and got[1][s * F:(s + 1) * F].tobytes() == rsm.tobytes()
    print(case["name"], "ids issued:", int(got[0].max()), "flags:", np.unique(got[2]).tolist())


@pytest.mark.parametrize("case", tr.GPU_CASES, ids=lambda c: c["name"])
def test_similarity_within_budget(tk, case):
    """The matrices of the frame in the middle of the clip, against the state the frames before it left."""
    clip = tr.case_clip(case)[0]
    K, P, T, S = case["K"], case["P"], case["T"], case["S"]
    F = len(clip[2]) // S
    f0 = F // 2
    t = tracker_for(tk, case)
    rows = np.concatenate([np.arange(s * F, s * F + f0) for s in range(S)])
    t.update_device(*(dev(p[rows]) for p in clip), frames_per_stream=f0)
    at = np.arange(S) * F + f0
    before = t.state.clone()
    sim = t.similarity_device(*(dev(p[at]) for p in clip)).cpu().numpy()
    assert torch.equal(before, t.state)
    worst = 0.0
    for s in range(S):
        ref = tr.Ref(K, P, T, **case.get("kw", {}))
        for f in range(f0):
            ref.step(*(p[s * F + f] for p in clip))
        j, sc, n, fl = (p[s * F + f0] for p in clip)
        want = ref.similarity(j, ref.valid_rows(j, sc, n, fl))
        worst = max(worst, float(np.abs(sim[s] - want).max()))
    print(f"{case['name']}: max |S_dev - S_numpy| = {worst:.3e}, budget {tr.sim_budget(K):.3e}")
    assert worst <= tr.sim_budget(K)


def test_assign_exact(tk):
    mats = tr.adversarial_matrices()
    clip = tr.case_clip(tr.GPU_CASES[2])[0]  # and a matrix of the host form: 30 people against their own tracks
    ref = tr.Ref(64, 30, 64)
    for f in range(3):
        ref.step(*(p[f] for p in clip))
    mats.append((ref.last_sim, ref.id.copy(), 0.3))
    for sim, ids, m in mats:
        got = tk.assign_device(dev(sim[None]), dev(ids[None]), m).cpu().numpy()[0]
        assert np.array_equal(got, tk.assign_host(sim[None], ids[None], m)[0]) and np.array_equal(got, tr.greedy(sim, ids, m))
    # several matrices in one launch
    sims, idss = np.stack([m[0] for m in mats[15:20]]), np.stack([m[1] for m in mats[15:20]])  # (the five 32 x 30 ones)
    assert np.array_equal(tk.assign_device(dev(sims), dev(idss), 0.3).cpu().numpy(), tk.assign_host(sims, idss, 0.3))


def test_chunking_invariance_and_repeat(tk):
    case = tr.GPU_CASES[0]  # 24 frames
    whole = dev_run(tk, case)
    assert same(whole, dev_run(tk, case, chunks=[1] * 24))
    assert same(whole, dev_run(tk, case, chunks=[5, 7, 12]))
    assert same(whole, dev_run(tk, case))  # two runs


@pytest.mark.parametrize("case", [tr.GPU_CASES[1], tr.GPU_CASES[3]], ids=lambda c: c["name"])
def test_streams_are_independent(tk, case):
    clip = tr.case_clip(case)[0]
    F = len(clip[2]) // case["S"]
    both = dev_run(tk, case)
    size = tk.state_bytes(case["K"], case["T"]) // 8
    for s in range(case["S"]):
        alone = dev_run(tk, case, tuple(p[s * F:(s + 1) * F] for p in clip), S=1)
        assert same([a[s * F:(s + 1) * F] for a in both[:3]], alone[:3])
        assert both[3][s * size:(s + 1) * size].tobytes() == alone[3].tobytes()


@pytest.mark.parametrize("case", [tr.GPU_CASES[0], tr.GPU_CASES[5]], ids=lambda c: c["name"])
def test_state_in_global_memory_gives_the_same_bits(tk, case):
    assert same(dev_run(tk, case), dev_run(tk, case, reserved=tk.STATE_GLOBAL))


def test_odd_element_offsets(tk, pkg):
    """Every buffer one element past a 16-byte boundary: the state 8 bytes, the float and int32 arrays 4 bytes."""
    case = tr.GPU_CASES[0]
    clip = tr.case_clip(case)[0]
    K, P, T, B = case["K"], case["P"], case["T"], len(clip[2])
    want = dev_run(tk, case)
    t = tracker_for(tk, case)
    nstate = t.state.numel()

    def odd(n, dtype):
        return torch.zeros(n + 4, dtype=dtype, device=DEV)[1:n + 1]
    state = odd(nstate, torch.int64)
    ins = [odd(p.size, torch.from_numpy(p).dtype).copy_(dev(p).reshape(-1)) for p in clip]
    ids, smooth, flags = odd(B * P, torch.int32), odd(B * P * K * 2, torch.float32), odd(B, torch.int32)
    assert all(a.data_ptr() % 16 in (4, 8) for a in [state, ids, smooth, flags] + ins)
    pkg._lib.launch(torch.device(DEV), pkg._lib.load().hh_track_step, C.byref(t.params), state.data_ptr(), *(a.data_ptr() for a in ins), 1, B,
                    ids.data_ptr(), smooth.data_ptr(), flags.data_ptr())
    assert same(want, [ids.cpu().numpy(), smooth.cpu().numpy(), flags.cpu().numpy(), state.cpu().numpy()])


def test_over_limit_call_is_refused_without_a_launch(tk, pkg):
    case = tr.GPU_CASES[0]
    clip = tr.case_clip(case)[0]
    t = tracker_for(tk, case)
    ins = [dev(p) for p in clip]
    B = len(clip[2])
    ids = torch.full((B, case["P"]), -7, dtype=torch.int32, device=DEV)
    smooth = torch.full((B, case["P"], case["K"], 2), -7.0, device=DEV)
    flags = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    lib = pkg._lib.load()
    for field, value in (("K", 65), ("max_tracks", 65), ("max_people", 65)):
        keep = getattr(t.params, field)
        setattr(t.params, field, value)
        with pytest.raises(pkg._lib.HHError, match="outside"):
            pkg._lib.launch(torch.device(DEV), lib.hh_track_step, C.byref(t.params), t.state.data_ptr(), *(a.data_ptr() for a in ins), 1, B,
                            ids.data_ptr(), smooth.data_ptr(), flags.data_ptr())
        setattr(t.params, field, keep)
    torch.cuda.synchronize()
    assert (ids == -7).all() and (smooth == -7).all() and (flags == -7).all() and not t.state.any()


@pytest.fixture(scope="module")
def model(pkg):
    net = pkg.HigherHRNet(17, 32)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 3)) for k, v in net.state_dict().items()})
    return pkg.InferenceKeypointsModel(net.to(DEV).eval(), det_thr=0.05, tag_thr=0.5, use_flip=False, input_size=128, device=DEV)


def test_end_to_end_video_frame_and_infer_images(tk, pkg, model):
    vz = importlib.import_module(PKG + ".keypoints.visualization")
    base = np.random.RandomState(4).randint(0, 255, (128, 128, 3)).astype(np.uint8)
    frames = [np.ascontiguousarray(np.roll(base, f, axis=1)) for f in range(6)]
    plain = model.infer_images(frames, max_batch=4)
    t1, t2 = tk.PoseTracker(device=DEV), tk.PoseTracker(device=DEV)
    live = [model.video_frame(f, tracker=t1) for f in frames]
    clip = model.infer_images(frames, max_batch=4, tracker=t2, render=dict(color_mode="track", alpha=0.65))
    tracked = 0
    for a, (b, out), c in zip(plain, live, clip):
        assert a.track_ids is None and a.kpts_coords_smooth is None
        for f in FIELDS:  # the results themselves are what they are without a tracker
            assert np.array_equal(getattr(a, f), getattr(b, f)) and np.array_equal(getattr(a, f), getattr(c, f)), f
        P = len(a.kpts_coords)
        assert b.track_ids.dtype == np.int32 and b.track_ids.shape == (P,) and b.kpts_coords_smooth.shape == a.kpts_coords.shape
        assert np.array_equal(b.track_ids, c.track_ids) and b.kpts_coords_smooth.tobytes() == c.kpts_coords_smooth.tobytes()
        assert out.shape == (640, 640, 3)
        table = vz.build_primitives(c.kpts_coords_smooth, c.kpts_scores, c.limbs, c.det_thr, "track", alpha=0.65, ids=c.track_ids)
        assert np.array_equal(c.rendered, vz.to_host(vz.render_frames_device([c.raw_image], [table], 0.65)[0]))
        tracked += int((b.track_ids != 0).sum())
    print("people:", [len(a.kpts_coords) for a in plain], "tracked rows:", tracked, "ids issued:", max(int(c.track_ids.max(initial=0)) for c in clip))
    assert torch.equal(t1.state, t2.state)
    with pytest.raises(ValueError):  # another model-input shape without a reset
        model.video_frame(np.zeros((128, 200, 3), np.uint8), tracker=t1)
    with pytest.raises(ValueError):  # a clip of mixed shapes
        model.infer_images([frames[0], np.zeros((128, 200, 3), np.uint8)], tracker=tk.PoseTracker(device=DEV))
    t1.reset()
    assert not t1.state.any()
    model.video_frame(np.zeros((128, 200, 3), np.uint8), tracker=t1)
