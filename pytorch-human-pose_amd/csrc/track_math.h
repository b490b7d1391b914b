// Pose tracking across frames (hh_track_* of include/hhrnet.h, where the rule is stated), kept apart from the kernel so that the same text
// also compiles for the host (hh_track_step_host, tools/track_host_check.cpp): the parameter block, the state's layout, the validity of a
// detection row, the similarity of one (track, detection) pair, the pieces of the greedy assignment, the slot bookkeeping, the One-Euro
// update of one joint, one frame of one stream in plain loops, the validation.
// Compile with -ffp-contract=off: every fp64 operation rounds on its own, so the exponent e_k and the whole filter are bit-identical to
// numpy's; only exp() may differ between the device, the host and numpy.  The assignment does no floating-point arithmetic, only
// comparisons, so given the same matrix it is exact.
#ifndef HH_TRACK_MATH_H
#define HH_TRACK_MATH_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/hhrnet.h"
#include "host_dev.h"

// One lane of one wave owns one track slot and the detections of a frame are a 64-bit set: the limits HH_TRACK_MAX_* are 64.
enum { TRACK_THREADS = 256 };
static_assert(HH_TRACK_MAX_TRACKS == 64 && HH_TRACK_MAX_PEOPLE == 64, "one wave of slots, a 64-bit set of detections");

using TrackParams = hh_track_params;  // passed to the kernel by value
static_assert(sizeof(hh_track_params) == 592, "ABI 3");

// One stream's state: header {issued ids, frames seen, 0, 0}, then per slot id / hits / misses / pad, the box area of the last matched
// pose, the filter's xhat and dxhat per coordinate, the last matched raw pose and its joint scores.  All zero = empty.
HH_HD int64_t track_state_bytes(int K, int T) { return ((int64_t)16 + 24 * (int64_t)T + 44 * (int64_t)T * K + 7) & ~(int64_t)7; }
struct TrackState {
    int32_t *hdr, *id, *hits, *misses;
    double *area, *xhat, *dxhat;  // [T], [T,K,2], [T,K,2]
    float *xy, *score;            // [T,K,2], [T,K]
};
HH_HD TrackState track_state_view(unsigned char *base, int K, int T)
{
    TrackState s;
    s.hdr = (int32_t *)base;
    s.id = s.hdr + 4;
    s.hits = s.id + T;
    s.misses = s.hits + T;
    s.area = (double *)(base + 16 + 16 * (size_t)T);
    s.xhat = s.area + T;
    s.dxhat = s.xhat + (size_t)T * K * 2;
    s.xy = (float *)(s.dxhat + (size_t)T * K * 2);
    s.score = s.xy + (size_t)T * K * 2;
    return s;
}

// A detection row is K joints of W floats: x, y, score and W - 3 more (3 + E in hh_decode's output; the kernel stages x, y, score: 3).
// Step 1: is row `det` with person score `person` a valid detection?
HH_HD bool track_det_valid(const float *det, int W, float person, const TrackParams &p)
{
    int n = 0;
    for (int k = 0; k < p.K; ++k) n += det[(size_t)k * W + 2] > p.joint_thr ? 1 : 0;
    return person >= p.min_person_score && n >= p.min_joints;
}

// Step 2: the similarity of a track's last matched raw pose and a detection.
// (Without a branch on the labels, so that the loads of one joint do not wait for each other: a joint that does not count adds an exact 0.)
HH_HD double track_similarity(const float *txy, const float *tscore, double area, const float *det, int W, const TrackParams &p)
{
    const double den = area + 2.220446049250313e-16;  // 2^-52
    double sum = 0.0;
    int n = 0;
    for (int k = 0; k < p.K; ++k) {
        const float *j = det + (size_t)k * W;
        const bool both = tscore[k] > p.joint_thr && j[2] > p.joint_thr;
        const double dx = (double)j[0] - (double)txy[2 * k], dy = (double)j[1] - (double)txy[2 * k + 1];
        const double e = ((dx * dx + dy * dy) / p.vars[k]) / den / 2.0;
        const double x = exp(-e);
        sum += both ? x : 0.0;
        n += both ? 1 : 0;
    }
    return (n >= p.min_common && n > 0) ? sum / (double)n : 0.0;
}

// The box area of a detection's labelled joints, not less than 1 (1 when none is labelled).
HH_HD double track_area(const float *det, int W, const TrackParams &p)
{
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    bool any = false;
    for (int k = 0; k < p.K; ++k) {
        const float *j = det + (size_t)k * W;
        const bool lab = j[2] > p.joint_thr;
        any = any || lab;
        const double x = (double)j[0], y = (double)j[1];
        x0 = lab && x < x0 ? x : x0; x1 = lab && x > x1 ? x : x1;
        y0 = lab && y < y0 ? y : y0; y1 = lab && y > y1 ? y : y1;
    }
    const double a = any ? (x1 - x0) * (y1 - y0) : 0.0;
    return a >= 1.0 ? a : 1.0;
}

// Step 3, one row: the best free detection of a track, the lowest d among equals; -1 when no free one reaches min_oks.
HH_HD int track_row_best(const double *row, int P, uint64_t taken, double min_oks, double *best)
{
    int bd = -1;
    double bs = 0.0;
    for (int d = 0; d < P; ++d) {  // (no branch around the load: the P loads of a row are in flight together)
        const double v = row[d];
        const bool take = !((taken >> d) & 1) && v >= min_oks && (bd < 0 || v > bs);
        bd = take ? d : bd;
        bs = take ? v : bs;
    }
    *best = bs;
    return bd;
}
// Step 3, between rows: is candidate a (similarity, track id, detection; d < 0 = none) taken before candidate b?
HH_HD bool track_better(double sa, int ida, int da, double sb, int idb, int db)
{
    if (da < 0) return false;
    if (db < 0) return true;
    if (sa != sb) return sa > sb;
    if (ida != idb) return ida < idb;
    return da < db;
}

// The index of the j-th (0-based) set bit of mask, -1 if there are fewer.
HH_HD int track_nth_bit(uint64_t mask, int j)
{
    for (int i = 0; i < j && mask; ++i) mask &= mask - 1;
    return mask ? __builtin_ctzll(mask) : -1;
}
HH_HD int track_popcount(uint64_t m)
{
    return __builtin_popcountll(m);
}

// Step 5 for one coordinate.  a_d = alpha(d_cutoff) for this Te.
HH_HD double track_alpha(double cutoff, double Te) { return 1.0 / (1.0 + (1.0 / ((2.0 * 3.141592653589793) * cutoff)) / Te); }
HH_HD void track_one_euro(double x, double Te, double a_d, const TrackParams &p, double *xhat, double *dxhat)
{
    const double dx = (x - *xhat) / Te;
    const double dh = a_d * dx + (1.0 - a_d) * *dxhat;
    const double c = p.min_cutoff + p.beta * fabs(dh);
    const double a = track_alpha(c, Te);
    *xhat = a * x + (1.0 - a) * *xhat;
    *dxhat = dh;
}

// Steps 4 and 5 for joint k of a row that holds track slot t: replaces the slot's raw pose, runs or restarts the filter, writes the
// row's smooth pair.  `fresh`: the track was opened in this frame.  Touches only element (t, k) of the state.
HH_HD void track_joint_update(const TrackState &st, int t, int k, const float *det, int W, bool fresh, double Te, double a_d, const TrackParams &p,
                               float *smooth)
{
    const float *j = det + (size_t)k * W;
    const size_t e = ((size_t)t * p.K + k) * 2;
    if (!(j[2] > p.joint_thr)) {  // unlabelled now: the last xy stays (a new track has none: the row's), with score 0
        st.score[(size_t)t * p.K + k] = 0.f;
        if (fresh) { st.xy[e] = j[0]; st.xy[e + 1] = j[1]; }
        smooth[0] = j[0];
        smooth[1] = j[1];
        return;
    }
    const bool was = !fresh && st.score[(size_t)t * p.K + k] > p.joint_thr;
    for (int c = 0; c < 2; ++c) {
        const double x = (double)j[c];
        if (!was) { st.xhat[e + c] = x; st.dxhat[e + c] = 0.0; }
        else track_one_euro(x, Te, a_d, p, &st.xhat[e + c], &st.dxhat[e + c]);
        smooth[c] = (float)st.xhat[e + c];
        st.xy[e + c] = j[c];
    }
    st.score[(size_t)t * p.K + k] = j[2];
}

// What a frame's wave decides for slot t, given the assignment (det = the matched detection or -1), the free-slot set (slots that are
// empty or expire in this frame) and the set of valid detections nobody matched: the j-th free slot takes the j-th such detection with
// id issued + j + 1.  Returns the detection the slot holds after this frame (-1: none) and updates the slot's header.
HH_HD int track_slot_update(const TrackState &st, int t, int det, uint64_t free_set, uint64_t unmatched, int issued, const float *joints_b, int W,
                             const TrackParams &p, bool *fresh, double *Te)
{
    *fresh = false;
    *Te = 0.0;
    if (det >= 0) {
        *Te = (double)(st.misses[t] + 1) / p.fps;
        st.hits[t] += 1;
        st.misses[t] = 0;
    } else if ((free_set >> t) & 1) {
        const int j = track_popcount(free_set & (((uint64_t)1 << t) - 1));
        det = track_nth_bit(unmatched, j);
        if (det >= 0) {
            st.id[t] = issued + j + 1;
            st.hits[t] = 1;
            st.misses[t] = 0;
            *fresh = true;
        } else if (st.id[t] != 0) {  // expired
            st.id[t] = 0;
            st.hits[t] = 0;
            st.misses[t] = 0;
        }
    } else {
        st.misses[t] += 1;
    }
    if (det >= 0) st.area[t] = track_area(joints_b + (size_t)det * p.K * W, W, p);
    return det;
}
HH_HD bool track_slot_free(const TrackState &st, int t, int det, const TrackParams &p)
{
    return st.id[t] == 0 || (det < 0 && st.misses[t] + 1 > p.max_age);
}

// Step 3 on the host: match[t] = the detection of track row t or -1.  ids[t] == 0: the row is not a live track.
inline void track_assign_host(const double *sim, const int32_t *ids, int T, int P, double min_oks, int32_t *match, uint64_t *taken_out)
{
    uint64_t taken = 0;
    for (int t = 0; t < T; ++t) match[t] = -1;
    for (;;) {
        double bs = 0.0;
        int bid = 0, bd = -1, bt = -1;
        for (int t = 0; t < T; ++t) {
            if (ids[t] == 0 || match[t] >= 0) continue;
            double s;
            const int d = track_row_best(sim + (size_t)t * P, P, taken, min_oks, &s);
            if (track_better(s, ids[t], d, bs, bid, bd)) { bs = s; bid = ids[t]; bd = d; bt = t; }
        }
        if (bd < 0) break;
        match[bt] = bd;
        taken |= (uint64_t)1 << bd;
    }
    if (taken_out) *taken_out = taken;
}

// The similarity matrix of one frame against a state: sim [T, P], 0 for an empty slot or an invalid row; valid_out = the valid rows.
inline uint64_t track_frame_valid_host(const TrackParams &p, const float *joints_b, const float *scores_b, int n, int flags)
{
    uint64_t valid = 0;
    if (flags & (HH_DECODE_FALLBACK | HH_DECODE_SOLVER_GUARD)) return 0;
    n = n < 0 ? 0 : (n > p.max_people ? p.max_people : n);
    for (int d = 0; d < n; ++d)
        if (track_det_valid(joints_b + (size_t)d * p.K * (3 + p.E), 3 + p.E, scores_b[d], p)) valid |= (uint64_t)1 << d;
    return valid;
}
inline void track_similarity_host(const TrackParams &p, const TrackState &st, const float *joints_b, uint64_t valid, double *sim)
{
    const int T = p.max_tracks, P = p.max_people;
    for (int t = 0; t < T; ++t)
        for (int d = 0; d < P; ++d)
            sim[(size_t)t * P + d] = (st.id[t] != 0 && ((valid >> d) & 1))
                                         ? track_similarity(st.xy + (size_t)t * p.K * 2, st.score + (size_t)t * p.K, st.area[t],
                                                            joints_b + (size_t)d * p.K * (3 + p.E), 3 + p.E, p)
                                         : 0.0;
}

// One frame of one stream on the host, what a workgroup does between two of its barriers.  sim: T * P doubles of scratch.
inline void track_frame_host(const TrackParams &p, unsigned char *state, const float *joints_b, const float *scores_b, int n, int flags,
                             int32_t *ids_b, float *smooth_b, int32_t *out_flags_b, double *sim)
{
    const int T = p.max_tracks, P = p.max_people, K = p.K;
    const TrackState st = track_state_view(state, K, T);
    const uint64_t valid = track_frame_valid_host(p, joints_b, scores_b, n, flags);
    track_similarity_host(p, st, joints_b, valid, sim);
    int32_t match[HH_TRACK_MAX_TRACKS];
    uint64_t taken = 0;
    track_assign_host(sim, st.id, T, P, p.min_oks, match, &taken);
    uint64_t free_set = 0;
    for (int t = 0; t < T; ++t)
        if (track_slot_free(st, t, match[t], p)) free_set |= (uint64_t)1 << t;
    const uint64_t unmatched = valid & ~taken;
    const int issued = st.hdr[0];
    int det_slot[HH_TRACK_MAX_PEOPLE];
    for (int d = 0; d < P; ++d) det_slot[d] = -1;
    bool fresh[HH_TRACK_MAX_TRACKS];
    double Te[HH_TRACK_MAX_TRACKS];
    for (int t = 0; t < T; ++t) {
        const int det = track_slot_update(st, t, match[t], free_set, unmatched, issued, joints_b, 3 + p.E, p, &fresh[t], &Te[t]);
        if (det >= 0) det_slot[det] = t;
    }
    const int nfree = track_popcount(free_set), nun = track_popcount(unmatched);
    st.hdr[0] = issued + (nun < nfree ? nun : nfree);
    st.hdr[1] += 1;
    *out_flags_b = (flags & HH_DECODE_SOLVER_GUARD ? HH_TRACK_SOLVER_GUARD : 0) | (nun > nfree ? HH_TRACK_POOL_FULL : 0);
    for (int d = 0; d < P; ++d) {
        const int t = det_slot[d];
        const float *det = joints_b + (size_t)d * K * (3 + p.E);
        ids_b[d] = t >= 0 ? st.id[t] : 0;
        const double a_d = t >= 0 && !fresh[t] ? track_alpha(p.d_cutoff, Te[t]) : 0.0;
        for (int k = 0; k < K; ++k) {
            float *o = smooth_b + ((size_t)d * K + k) * 2;
            if (t >= 0) track_joint_update(st, t, k, det, 3 + p.E, fresh[t], Te[t], a_d, p, o);
            else { o[0] = det[(size_t)k * (3 + p.E)]; o[1] = det[(size_t)k * (3 + p.E) + 1]; }
        }
    }
}

// What the hh_track_* entry points refuse in the parameter block; nullptr when accepted.
inline const char *track_check(const TrackParams *p)
{
    if (!p) return "null pointer";
    if (p->K < 1 || p->K > HH_TRACK_MAX_K) return "K outside 1..HH_TRACK_MAX_K (64)";
    if (p->max_tracks < 1 || p->max_tracks > HH_TRACK_MAX_TRACKS) return "max_tracks outside 1..HH_TRACK_MAX_TRACKS (64)";
    if (p->max_people < 1 || p->max_people > HH_TRACK_MAX_PEOPLE) return "max_people outside 1..HH_TRACK_MAX_PEOPLE (64)";
    if (p->E < 0 || p->E > 64) return "E outside 0..64";
    for (int k = 0; k < p->K; ++k)
        if (!(p->vars[k] > 0.0) || !isfinite(p->vars[k])) return "vars must be finite and > 0";
    if (!(p->fps > 0.0) || !isfinite(p->fps)) return "fps must be finite and > 0";
    if (!(p->min_cutoff > 0.0) || !isfinite(p->min_cutoff)) return "min_cutoff must be finite and > 0";
    if (!(p->d_cutoff > 0.0) || !isfinite(p->d_cutoff)) return "d_cutoff must be finite and > 0";
    if (!(p->beta >= 0.0) || !isfinite(p->beta)) return "beta must be finite and >= 0";
    if (p->max_age < 0) return "max_age must be >= 0";
    if (!(p->min_oks > 0.0) || !(p->min_oks <= 1.0)) return "min_oks outside (0, 1]";
    if (!(p->joint_thr >= 0.f) || !isfinite(p->joint_thr)) return "joint_thr must be finite and >= 0";
    if (p->min_person_score != p->min_person_score) return "min_person_score is NaN";
    if (p->min_joints < 0 || p->min_common < 0) return "min_joints and min_common must be >= 0";
    return nullptr;
}
#endif
