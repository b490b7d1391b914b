"""Shared by tests/test_track_cpu.py and tests/test_gpu_track.py: a numpy float64 restatement of the tracking rule (hh_track_step in
include/hhrnet.h), a seeded generator of synthetic clips rendered directly as decode outputs, a DERIVED error budget for the similarity,
and the margin of a clip, which makes "exactly equal ids" a fair demand on a similarity that may differ in its last bits.

The budget (sim_budget).  For one (track, detection) pair the restatement and the code under test (csrc/track_math.h on the host or on
the device) both form, per joint k labelled in both,
    e_k = ((dx*dx + dy*dy) / vars_k) / (area + 2^-52) / 2
in fp64 from the same float32 operands with every operation rounded on its own and in the same order (the library is built with
-ffp-contract=off), so e_k is bit-identical BY CONSTRUCTION whatever its magnitude, and e_k >= 0 so x_k = exp(-e_k) lies in [0, 1].
(Beyond e_k ~ 708 x_k is subnormal or 0 and an ulp bound no longer holds relatively; its absolute error is then below 2^-1022.)
The two sides differ in three places only:
  * x_k = exp(-e_k): each library is within its documented bound of the true value.  numpy's float64 exp is glibc's (1 ulp), numpy's
    AVX512F kernel (0.52 ulp) or an SVML routine (numpy holds those to 4 ulp): ULP_EXP_NUMPY = 4 is taken.  The device's exp is OCML's
    (ROCm "HIP math API", double precision exp: 1 ulp), compiled for the host the header calls glibc's (1 ulp): ULP_EXP_TEST = 1.
    ulp(x_k) <= 2u x_k <= 2u, u = 2^-53.
  * the sum of the n <= K terms, on both sides in ascending k (np.cumsum adds sequentially; a term that does not count is an exact + 0):
    each side is within gamma_(n-1) * n of the exact sum of ITS terms, gamma_m = m u / (1 - m u) (Higham, section 4.2).
  * the division by n: one rounding on each side of a value <= 1: u each.
So |S_ref - S_test| <= [ n (ULP_EXP_NUMPY + ULP_EXP_TEST) 2u + 2 gamma_(n-1) n ] / n + 2u, largest at n = K.  Nothing in it comes from
running the code under test.

The margin (Ref.margin).  Ids can only be required to be EQUAL where no decision of the greedy assignment hangs on the last bits of a
similarity: the smallest |S - min_oks| over all (live track, valid detection) pairs of all frames, and the smallest gap between two
candidates (S >= min_oks) that share a track or a detection.  The tests require 1000 budgets of it from every clip they use, on the
restatement alone; hh_track_assign itself must not depend on it and gets adversarial matrices.
"""
import numpy as np

ULP_EXP_NUMPY, ULP_EXP_TEST = 4.0, 1.0
U = 2.0 ** -53
FALLBACK, GUARD, POOL_FULL = 1, 2, 4
PI = 3.141592653589793
COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
DEFAULTS = dict(min_oks=0.3, max_age=30, joint_thr=0.05, min_joints=3, min_common=3, min_person_score=0.0, fps=30.0, min_cutoff=1.0, beta=0.007,
                d_cutoff=1.0)


def sigmas_for(K: int) -> np.ndarray:
    return COCO_SIGMAS if K == 17 else 0.03 + 0.01 * (np.arange(K) % 7)


def sim_budget(K: int) -> float:
    g = (K - 1) * U / (1 - (K - 1) * U)
    return (ULP_EXP_NUMPY + ULP_EXP_TEST) * 2 * U + 2 * g + 2 * U


def greedy(sim: np.ndarray, ids: np.ndarray, min_oks: float) -> np.ndarray:
    """Step 3 on one matrix [T,P]: candidates S >= min_oks in descending S, then ascending track id, then ascending d."""
    T, P = sim.shape
    cand = [(-sim[t, d], int(ids[t]), d, t) for t in range(T) if ids[t] != 0 for d in range(P) if sim[t, d] >= min_oks]
    cand.sort()
    match = np.full(T, -1, np.int32)
    used = set()
    for _, _, d, t in cand:
        if match[t] < 0 and d not in used:
            match[t] = d
            used.add(d)
    return match


class Ref:
    """One stream.  step() takes one frame of decode outputs (float32 joints [P,K,3+E], scores [P], n, flags)."""

    def __init__(self, K, max_people, max_tracks, sigmas=None, **kw):
        self.K, self.P, self.T = K, max_people, max_tracks
        self.p = dict(DEFAULTS, **kw)
        self.vars = (np.asarray(sigmas_for(K) if sigmas is None else sigmas, np.float64) * 2) ** 2
        self.thr = np.float32(self.p["joint_thr"])
        T = max_tracks
        self.issued, self.frames = 0, 0
        self.id, self.hits, self.misses = np.zeros(T, np.int32), np.zeros(T, np.int32), np.zeros(T, np.int32)
        self.area = np.zeros(T)
        self.xy, self.score = np.zeros((T, K, 2), np.float32), np.zeros((T, K), np.float32)
        self.xhat, self.dxhat = np.zeros((T, K, 2)), np.zeros((T, K, 2))
        self.margin = np.inf
        self.last_sim = None

    def valid_rows(self, joints, scores, n, flags):
        if flags & (FALLBACK | GUARD):
            return np.zeros(self.P, bool)
        lab = joints[:, :, 2] > self.thr
        ok = (scores >= np.float32(self.p["min_person_score"])) & (lab.sum(1) >= self.p["min_joints"])
        return ok & (np.arange(self.P) < min(max(int(n), 0), self.P))

    def similarity(self, joints, valid):
        """[T,P] float64; 0 for an empty slot or an invalid row."""
        live = self.id != 0
        tl = self.score > self.thr                                   # [T,K]
        dl = joints[:, :, 2] > self.thr                              # [P,K]
        common = tl[:, None, :] & dl[None, :, :]
        dx = joints[None, :, :, 0].astype(np.float64) - self.xy[:, None, :, 0].astype(np.float64)
        dy = joints[None, :, :, 1].astype(np.float64) - self.xy[:, None, :, 1].astype(np.float64)
        den = np.where(live, self.area, 1.0) + 2.220446049250313e-16
        e = ((dx * dx + dy * dy) / self.vars[None, None, :]) / den[:, None, None] / 2.0
        x = np.where(common, np.exp(-e), 0.0)
        n = common.sum(-1)
        s = np.cumsum(x, axis=-1)[..., -1] / np.maximum(n, 1)
        s = np.where((n >= self.p["min_common"]) & (n > 0), s, 0.0)
        return np.where(live[:, None] & valid[None, :], s, 0.0)

    def _note_margin(self, sim, valid):
        live = self.id != 0
        m = self.p["min_oks"]
        vals = sim[np.ix_(live, valid)]
        if vals.size:
            self.margin = min(self.margin, float(np.abs(vals - m).min()))
        full = np.where(live[:, None] & valid[None, :] & (sim >= m), sim, np.nan)
        for lines in (full, full.T):
            for row in lines:
                c = np.sort(row[~np.isnan(row)])
                if len(c) > 1:
                    self.margin = min(self.margin, float(np.diff(c).min()))

    def alpha(self, c, Te):
        return 1.0 / (1.0 + (1.0 / ((2.0 * PI) * c)) / Te)

    def step(self, joints, scores, n, flags=0):
        p, K, P, T = self.p, self.K, self.P, self.T
        joints, scores = np.asarray(joints, np.float32), np.asarray(scores, np.float32)
        valid = self.valid_rows(joints, scores, n, flags)
        sim = self.similarity(joints, valid)
        self.last_sim = sim
        self._note_margin(sim, valid)
        match = greedy(sim, self.id, p["min_oks"])
        taken = np.zeros(P, bool)
        taken[match[match >= 0]] = True
        free = (self.id == 0) | ((match < 0) & (self.misses + 1 > p["max_age"]))
        unmatched = np.nonzero(valid & ~taken)[0]
        free_slots = np.nonzero(free)[0]
        det_of, fresh, Te = match.copy(), np.zeros(T, bool), np.zeros(T)
        for t in range(T):
            if match[t] >= 0:
                Te[t] = np.float64(int(self.misses[t]) + 1) / np.float64(p["fps"])
                self.hits[t] += 1
                self.misses[t] = 0
            elif free[t]:
                j = int(np.searchsorted(free_slots, t))
                if j < len(unmatched):
                    det_of[t] = unmatched[j]
                    self.id[t], self.hits[t], self.misses[t], fresh[t] = self.issued + j + 1, 1, 0, True
                else:
                    self.id[t] = self.hits[t] = self.misses[t] = 0
            else:
                self.misses[t] += 1
        nnew = min(len(unmatched), len(free_slots))
        self.issued += nnew
        self.frames += 1
        out_flags = (GUARD if flags & GUARD else 0) | (POOL_FULL if len(unmatched) > len(free_slots) else 0)
        ids = np.zeros(P, np.int32)
        smooth = joints[:, :, :2].copy()
        for t in range(T):
            d = det_of[t]
            if d < 0:
                continue
            ids[d] = self.id[t]
            lab = joints[d, :, 2] > self.thr
            xy64 = joints[d, :, :2].astype(np.float64)
            pts = xy64[lab]
            a = (pts[:, 0].max() - pts[:, 0].min()) * (pts[:, 1].max() - pts[:, 1].min()) if len(pts) else 0.0
            self.area[t] = a if a >= 1.0 else 1.0
            was = np.zeros(K, bool) if fresh[t] else (self.score[t] > self.thr)
            run, start = lab & was, lab & ~was
            if run.any():
                a_d = self.alpha(np.float64(p["d_cutoff"]), Te[t])
                x, xh, dh = xy64[run], self.xhat[t, run], self.dxhat[t, run]
                dxv = (x - xh) / Te[t]
                dnew = a_d * dxv + (1.0 - a_d) * dh
                c = np.float64(p["min_cutoff"]) + np.float64(p["beta"]) * np.fabs(dnew)
                al = self.alpha(c, Te[t])
                self.xhat[t, run] = al * x + (1.0 - al) * xh
                self.dxhat[t, run] = dnew
            self.xhat[t, start] = xy64[start]
            self.dxhat[t, start] = 0.0
            smooth[d, lab] = self.xhat[t, lab].astype(np.float32)
            keep = lab | fresh[t]
            self.xy[t, keep] = joints[d, keep, :2]
            self.score[t] = np.where(lab, joints[d, :, 2], np.float32(0))
        return ids, smooth, np.int32(out_flags)


def run_ref(clip, K, max_people, max_tracks, **kw):
    """The restatement over a clip (joints [F,P,K,3+E], scores [F,P], num [F], flags [F]) -> (ids, smooth, out_flags, Ref)."""
    joints, scores, num, flags = clip
    ref = Ref(K, max_people, max_tracks, **kw)
    out = [ref.step(joints[f], scores[f], num[f], flags[f]) for f in range(len(num))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int32), ref


def make_clip(seed, K, max_people, frames, people=None, E=1, size=512.0, toggle=True, always=False):
    """`people` (default: 1..6 by the seed) persons on smooth real-valued trajectories with per-joint jitter, present over an interval
    of the clip (the whole of it with `always`), their rows shuffled in every frame, some joints dropping below the label threshold for a few frames.
    -> (joints float32 [F,P,K,3+E], scores float32 [F,P], num int32 [F], flags int32 [F] = 0)."""
    rs = np.random.RandomState(seed)
    n = int(rs.randint(1, 7)) if people is None else int(people)
    n = min(n, max_people)
    joints = np.zeros((frames, max_people, K, 3 + E), np.float32)
    scores = np.zeros((frames, max_people), np.float32)
    num = np.zeros(frames, np.int32)
    # a grid of home cells keeps different people apart (similarities between them stay far below min_oks)
    cells = int(np.ceil(np.sqrt(max(n, 1))))
    cell = size / cells
    order = rs.permutation(cells * cells)[:n]
    persons = []
    for i in range(n):
        cy, cx = divmod(int(order[i]), cells)
        h = cell * rs.uniform(0.35, 0.5)
        persons.append(dict(c0=np.array([(cx + 0.5) * cell, (cy + 0.5) * cell]), v=rs.uniform(-0.2, 0.2, 2) * cell / frames, amp=rs.uniform(0.02, 0.08, 2) * cell,
                            w=rs.uniform(0.1, 0.4, 2), ph=rs.uniform(0, 6.28, 2), shape=rs.uniform(-0.5, 0.5, (K, 2)) * np.array([0.5 * h, h]),
                            first=0 if always or n <= 2 or i == 0 else int(rs.randint(0, frames // 3 + 1)), last=frames if always or n <= 2 or i == 0 else int(rs.randint(2 * frames // 3, frames + 1)),
                            tag=rs.normal(0, 2.0, E), off=(int(rs.randint(0, K)), int(rs.randint(2, frames)), int(rs.randint(1, 4)))))
    for f in range(frames):
        rows = []
        for q in persons:
            if not q["first"] <= f < q["last"]:
                continue
            c = q["c0"] + q["v"] * f + q["amp"] * np.sin(q["w"] * f + q["ph"])
            xy = c + q["shape"] + rs.normal(0, 0.3, (K, 2))
            sc = rs.uniform(0.3, 0.95, K)
            k0, f0, ln = q["off"]
            if toggle and f0 <= f < f0 + ln:
                sc[k0] = 0.01
            rows.append((xy, sc, q["tag"]))
        for r, i in enumerate(rs.permutation(len(rows))):
            xy, sc, tag = rows[i]
            joints[f, r, :, :2], joints[f, r, :, 2], joints[f, r, :, 3:] = xy, sc, tag + rs.normal(0, 0.05, (K, E))
            scores[f, r] = sc.mean()
        num[f] = len(rows)
    return joints, scores, num, np.zeros(frames, np.int32)


def host_run(tk, clip, K, P, T, S=1, chunks=None, **kw):
    """The clip through hh_track_step_host in `chunks` (default: one call) -> (ids, smooth, flags, state)."""
    joints, scores, num, flags = clip
    F = len(num) // S
    params = tk.make_params(K, P, T, kw.pop("sigmas", sigmas_for(K)), E=joints.shape[-1] - 3, **dict(DEFAULTS, **kw))
    state = np.zeros(S * tk.state_bytes(K, T) // 8, np.int64)
    outs = []
    at = 0
    for n in chunks or [F]:
        sel = np.concatenate([np.arange(s * F + at, s * F + at + n) for s in range(S)])
        o = tk.step_host(params, state, joints[sel], scores[sel], num[sel], flags[sel], n)
        outs.append([a.reshape((S, n) + a.shape[1:]) for a in o])
        at += n
    return [np.concatenate([o[i] for o in outs], 1).reshape((S * F,) + outs[0][i].shape[2:]) for i in range(3)] + [state]


# ------------------------------------------------------------------------------------------------ the clips of the GPU tests
# The smallest shapes at which the kernel can go wrong: K and max_tracks at 5 / 17 / 64 and 4 / 32 / 64, max_people = 30 with 0, 1, a few
# and 30 people per frame, one and three streams, a pool smaller than the crowd, a state that fits LDS below 64 KB (K17 / K5), one that
# needs the large LDS window (K64-T32: 119 KB with the similarities and the staged rows) and one that stays in global memory (K64-T64: 176 KB of state).
GPU_CASES = [
    dict(name="K17-T32-S1", seed=1, K=17, T=32, P=30, S=1, people=5, frames=24),
    dict(name="K5-T4-S3-poolfull", seed=2, K=5, T=4, P=30, S=3, people=6, frames=12),
    dict(name="K64-T64-S1-30people", seed=3, K=64, T=64, P=30, S=1, people=30, frames=12),
    dict(name="K17-T64-S3-1person", seed=4, K=17, T=64, P=30, S=3, people=1, frames=40),
    dict(name="K5-T32-S1-0people", seed=5, K=5, T=32, P=30, S=1, people=0, frames=12),
    dict(name="K64-T32-S1", seed=6, K=64, T=32, P=30, S=1, people=3, frames=16, kw=dict(max_age=2)),
]
_CACHE = {}


def case_clip(case):
    """-> (clip of S * frames rows, stream-major; [run_ref(...) of each stream]).  Computed once per case and shared: treat as read-only."""
    if case["name"] not in _CACHE:
        streams = [make_clip(case["seed"] * 100 + s, case["K"], case["P"], case["frames"], case["people"]) for s in range(case["S"])]
        refs = [run_ref(c, case["K"], case["P"], case["T"], **case.get("kw", {})) for c in streams]
        _CACHE[case["name"]] = (tuple(np.concatenate(part) for part in zip(*streams)), refs)
    return _CACHE[case["name"]]


def adversarial_matrices():
    """(sim [T,P], ids [T], min_oks) that violate the margin condition on purpose: exact ties in rows, in columns and across both,
    everything equal, values exactly at min_oks and one ulp below it, dead rows with large values."""
    rs = np.random.RandomState(5)
    out = []
    for T, P in ((4, 4), (7, 3), (3, 9), (32, 30), (64, 64), (1, 1)):
        ids = (rs.permutation(T + 3)[:T] + 1).astype(np.int32)
        ids[rs.rand(T) < 0.2] = 0
        out.append((np.full((T, P), 0.5), ids, 0.5))
        out.append((np.full((T, P), np.nextafter(0.5, 0)), ids, 0.5))
        out.append((rs.randint(0, 4, (T, P)) / 4.0, ids, 0.25))          # few distinct values: ties everywhere
        m = rs.rand(T, P)
        m[:, 0] = m[0, 0]
        m[T // 2] = m[0, 0]
        out.append((m, ids, 0.3))
        out.append((rs.rand(T, P), ids, 0.3))
    return out
