"""Pose tracking without a GPU: hh_track_step_host (csrc/track_math.h compiled for the host) against the numpy restatement of
tests/track_ref.py, the margin condition of every clip the GPU tests use, the greedy assignment on adversarial matrices, the lifecycle
of a track, every refusal, and the "track" colour table of build_primitives."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import track_ref as tr
from conftest import GOLDEN, PKG


@pytest.fixture(scope="module")
def tk():
    return importlib.import_module(PKG + ".keypoints.tracking")


@pytest.mark.parametrize("case", tr.GPU_CASES, ids=lambda c: c["name"])
def test_host_equals_numpy_and_margin(tk, case):
    clip, refs = tr.case_clip(case)
    K, P, T, S = case["K"], case["P"], case["T"], case["S"]
    margin = min(r[3].margin for r in refs)
    print(f"{case['name']}: margin {margin:.3e}, budget {tr.sim_budget(K):.3e}")
    assert margin >= 1000 * tr.sim_budget(K)
    ids, smooth, flags, _ = tr.host_run(tk, clip, K, P, T, S, **case.get("kw", {}))
    F = len(clip[2]) // S
    for s, (rid, rsm, rfl, _) in enumerate(refs):
        sl = slice(s * F, (s + 1) * F)
        assert np.array_equal(ids[sl], rid)
        assert np.array_equal(flags[sl], rfl)
        assert smooth[sl].tobytes() == rsm.tobytes()
    if case["people"] != 0:
        assert ids.max() > 0


def test_host_chunking_invariance(tk):
    case = tr.GPU_CASES[0]
    clip, _ = tr.case_clip(case)
    a = tr.host_run(tk, clip, case["K"], case["P"], case["T"])
    b = tr.host_run(tk, clip, case["K"], case["P"], case["T"], chunks=[5, 7, 12])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_assign_adversarial(tk):
    for sim, ids, min_oks in tr.adversarial_matrices():
        got = tk.assign_host(sim[None], ids[None], min_oks)[0]
        assert np.array_equal(got, tr.greedy(sim, ids, min_oks)), (sim, ids)
    # everything equal: track ids ascending take detections ascending, whatever their slots
    sim = np.full((4, 3), 0.5)
    assert tk.assign_host(sim[None], np.array([[7, 2, 0, 5]], np.int32), 0.5)[0].tolist() == [2, 0, -1, 1]
    # an exact tie between two tracks for one detection goes to the lower id, the loser falls back on its next best
    sim = np.array([[0.9, 0.4], [0.9, 0.0]])
    assert tk.assign_host(sim[None], np.array([[2, 1]], np.int32), 0.3)[0].tolist() == [1, 0]


def one_person(K, P, frames, present, xy0=(100.0, 120.0), step=1.0, E=1):
    """A rigid person moving right by `step` px per frame, in row 0 of the frames listed in `present`."""
    rs = np.random.RandomState(3)
    shape = rs.uniform(-30, 30, (K, 2))
    joints, scores, num = np.zeros((frames, P, K, 3 + E), np.float32), np.zeros((frames, P), np.float32), np.zeros(frames, np.int32)
    for f in present:
        joints[f, 0, :, :2] = np.array(xy0) + shape + [step * f, 0]
        joints[f, 0, :, 2] = 0.8
        scores[f, 0], num[f] = 0.8, 1
    return joints, scores, num, np.zeros(frames, np.int32)


def both(tk, clip, K, P, T, **kw):
    ids, smooth, flags, state = tr.host_run(tk, clip, K, P, T, **kw)
    rid, rsm, rfl, ref = tr.run_ref(clip, K, P, T, **kw)
    assert np.array_equal(ids, rid) and np.array_equal(flags, rfl) and smooth.tobytes() == rsm.tobytes()
    return ids, smooth, flags, state


@pytest.mark.parametrize("gap,same", [(3, True), (4, False)])
def test_expiry_exactly_at_max_age(tk, gap, same):
    """max_age = 3: a track missed 3 times is still matched, one missed 4 times has been freed and its id is not used again."""
    frames = gap + 2
    clip = one_person(5, 4, frames, [0, frames - 1], step=0.25)
    ids = both(tk, clip, 5, 4, 4, max_age=3)[0]
    assert ids[0, 0] == 1 and ids[-1, 0] == (1 if same else 2)
    assert (ids[1:-1] == 0).all()


def test_ids_never_reused_and_pool_full(tk):
    K, P, T = 5, 8, 2
    clip = tr.make_clip(11, K, P, 12, people=4, toggle=False, always=True)
    ids, _, flags, state = both(tk, clip, K, P, T, max_age=1)
    assert (flags == tr.POOL_FULL).all()  # 4 people, 2 slots: two rows stay without an id in every frame
    assert ((ids != 0).sum(1) == 2).all() and set(np.unique(ids)) == {0, 1, 2}
    # the two tracked people leave: their slots expire and the others get NEW ids
    joints, scores, num, fl = clip
    keep = (ids[-1] == 0) & (np.arange(P) < 4)
    j2, s2 = np.zeros_like(joints), np.zeros_like(scores)
    j2[:, :2], s2[:, :2] = joints[-1:, keep], scores[-1:, keep]
    clip2 = tuple(np.concatenate(p) for p in zip(clip, (j2, s2, np.full(12, 2, np.int32), fl)))
    ids2 = both(tk, clip2, K, P, T, max_age=1)[0]
    # (max_age = 1: missed once in frame 12, freed by the second miss in frame 13, and a slot freed in a frame is open in that frame)
    assert ids2[12].max() == 0 and all(sorted(r[:2]) == [3, 4] for r in ids2[13:].tolist())


def test_fallback_guard_and_empty_frames(tk):
    K, P, T = 5, 4, 4
    clip = one_person(K, P, 8, range(8))
    clip[3][2], clip[3][4] = tr.FALLBACK, tr.GUARD
    clip[2][6] = 0
    ids, smooth, flags, _ = both(tk, clip, K, P, T)
    assert ids[:, 0].tolist() == [1, 1, 0, 1, 0, 1, 0, 1]
    assert flags.tolist() == [0, 0, 0, 0, tr.GUARD, 0, 0, 0]
    for f in (2, 4, 6):  # rows without a track carry the raw coordinates
        assert np.array_equal(smooth[f], clip[0][f, :, :, :2])


def test_label_toggle_restarts_filter(tk):
    K, P, T = 5, 4, 4
    clip = one_person(K, P, 6, range(6), step=3.0)
    clip[0][3, 0, 2, 2] = 0.01  # joint 2 unlabelled in frame 3
    ids, smooth, _, _ = both(tk, clip, K, P, T)
    raw = clip[0][:, 0, :, :2]
    assert (ids[:, 0] == 1).all()
    assert np.array_equal(smooth[0, 0], raw[0])                    # a new track starts at the raw pose
    assert (smooth[2, 0, :, 0] < raw[2, :, 0]).all()               # the filter lags a moving joint
    assert np.array_equal(smooth[3, 0, 2], raw[3, 2])              # unlabelled: raw
    assert np.array_equal(smooth[4, 0, 2], raw[4, 2])              # labelled again: starts afresh
    assert (smooth[4, 0, [0, 1, 3, 4], 0] < raw[4, [0, 1, 3, 4], 0]).all()


BAD_PARAMS = [dict(K=65), dict(K=0), dict(T=65), dict(P=65), dict(vars0=0.0), dict(vars0=float("inf")), dict(vars0=float("nan")), dict(fps=0.0),
              dict(fps=float("inf")), dict(min_cutoff=-1.0), dict(min_cutoff=float("nan")), dict(d_cutoff=0.0), dict(beta=-0.1), dict(max_age=-1),
              dict(min_oks=0.0), dict(min_oks=1.5), dict(min_oks=float("nan")), dict(joint_thr=-0.1)]


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_refusals_params(tk, pkg, bad):
    lib = pkg._lib.load()
    params = tk.make_params(5, 4, 4, tr.sigmas_for(5), **dict(tr.DEFAULTS, **{k: v for k, v in bad.items() if k in tr.DEFAULTS}))
    params.K, params.max_tracks, params.max_people = bad.get("K", 5), bad.get("T", 4), bad.get("P", 4)
    if "vars0" in bad:
        params.vars[2] = bad["vars0"]
    buf = np.zeros(1 << 16, np.float64)
    a = buf.ctypes.data
    assert lib.hh_track_step_host(C.byref(params), a, a, a, a, None, 1, 1, a, a, a) == 1
    assert lib.hh_track_step(C.byref(params), a, a, a, a, None, 1, 1, a, a, a, None) == 1  # refused before any launch: no GPU is touched
    assert lib.hh_track_similarity(C.byref(params), a, a, a, a, None, 1, a, None) == 1
    assert lib.hh_last_error()


def test_refusals_pointers_and_limits(tk, pkg):
    lib = pkg._lib.load()
    params = tk.make_params(5, 4, 4, tr.sigmas_for(5), **tr.DEFAULTS)
    buf = np.zeros(1 << 12, np.float64)
    a = buf.ctypes.data
    ok = [C.byref(params), a, a, a, a, None, 0, 1, a, a, a]
    assert lib.hh_track_step_host(*ok) == 0
    for i in (0, 1, 2, 3, 4, 8, 9, 10):  # each pointer null
        args = list(ok)
        args[i] = None
        assert lib.hh_track_step_host(*args) == 1 and lib.hh_track_step(*args, None) == 1
    for i, off in ((1, 4), (2, 2), (3, 1), (4, 2), (5, 2), (8, 2), (9, 1), (10, 3)):  # each pointer misaligned
        args = list(ok)
        args[i] = a + off
        assert lib.hh_track_step_host(*args) == 1 and lib.hh_track_step(*args, None) == 1
    assert lib.hh_track_state_bytes(65, 4) == -1 and lib.hh_track_state_bytes(5, 65) == -1 and lib.hh_track_state_bytes(17, 64) > 0
    assert lib.hh_track_reset(None, 5, 4, 1, None) == 1 and lib.hh_track_reset(a + 4, 5, 4, 1, None) == 1 and lib.hh_track_reset(a, 65, 4, 1, None) == 1
    sim = [a, a, 1, 4, 4, 0.3, a]
    assert lib.hh_track_assign_host(*sim) == 0
    for i, v in ((0, None), (1, None), (6, None), (0, a + 4), (1, a + 2), (6, a + 2), (3, 65), (4, 65), (3, 0), (5, 0.0), (5, 1.5), (5, float("nan"))):
        args = list(sim)
        args[i] = v
        assert lib.hh_track_assign_host(*args) == 1 and lib.hh_track_assign(*args, None) == 1


def test_build_primitives_track_table(pkg):
    vz = importlib.import_module(PKG + ".keypoints.visualization")
    g = np.load(os.path.join(GOLDEN, "track_primitives.npz"))
    coords, scores, limbs = g["coords"], g["scores"], [tuple(l) for l in g["limbs"]]
    for mode in ("person", "limb"):  # tables recorded before "track" existed
        assert vz.build_primitives(coords, scores, limbs, 0.05, mode).view(np.uint8).tobytes() == g[mode].tobytes()
    ids = np.array([3, 0, 1, 103, 2], np.int32)
    table = vz.build_primitives(coords, scores, limbs, 0.05, "track", ids=ids)
    # the same rows as "person" on the tracked people in palette order (id - 1) % 100: the palette permuted accordingly
    keep = ids != 0
    pal = np.zeros((4, 3), np.uint8)
    pal[:] = vz.DEFAULT_PALETTE[(ids[keep] - 1) % len(vz.DEFAULT_PALETTE)]
    want = vz.build_primitives(coords[keep], scores[keep], limbs, 0.05, "person", palette=pal)
    assert table.tobytes() == want.tobytes() and len(table) > 0
    assert (table["rgb"][table["kind"] != vz.RING][0] == vz.DEFAULT_PALETTE[2]).all()
    assert len(vz.build_primitives(coords, scores, limbs, 0.05, "track", ids=np.zeros(5, np.int32))) == 0
    with pytest.raises(ValueError):
        vz.build_primitives(coords, scores, limbs, 0.05, "track")
