// Per-image OKS / PCKh against annotations (hh_pose_score_batch of include/hhrnet.h, whose text is the specification), kept apart from the
// kernel so that the same text also compiles for the host (hh_pose_score_host, tools/pose_score_host_check.cpp): the tables, the un-warp of
// one prediction coordinate, the walk rank, D of one (prediction, target) pair, the per-joint term, one image in plain loops, the
// validation, the polygon area.  Compile with -ffp-contract=off: every fp64 operation rounds on its own, so everything in front of exp()
// is bit-identical on both sides; only exp() itself may differ.
#ifndef HH_POSE_SCORE_MATH_H
#define HH_POSE_SCORE_MATH_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/hhrnet.h"
#include "host_dev.h"

// One workgroup owns one image.  Its un-warped predictions live in LDS ([P,K,2] fp64, 64 KB at the maxima), each of its POSE_WAVES waves
// owns one target at a time (the target's row [K,3] and its K terms staged per wave); lane p of the wave holds D[p,t], so P <= 64 = one
// wave, and lane k holds joint k's term, so K <= 64.
enum { POSE_THREADS = 256, POSE_WAVES = POSE_THREADS / 64 };
static_assert(HH_POSE_MAX_P == 64 && HH_POSE_MAX_K <= 64, "one lane per prediction, one lane per joint");

// The arguments of one call as the kernel takes them (by value: vars rides in the launch's arguments).  Not part of the ABI.
struct PoseTables {
    const float *joints, *scores;
    const int32_t *num, *flags;
    const double *inv_affine;
    const int32_t *p_off;
    const double *p_xy, *p_score;
    const int32_t *t_off;
    const double *t_xyv, *t_area, *t_head;
    double vars[HH_POSE_MAX_K];
    double alpha;
    int64_t image_stride, person_stride, joint_stride, score_stride;
    int32_t B, K, form, metric, max_people;
};

HH_HD size_t pose_lds_bytes(int P, int K) { return ((size_t)P * K * 2 + (size_t)POSE_WAVES * K * 4) * sizeof(double); }

HH_HD bool pose_finite(double v) { return v - v == 0.0; }
HH_HD double pose_nan() { return __builtin_nan(""); }

HH_HD int pose_num_preds(const PoseTables &t, int i)
{
    if (t.form == HH_POSE_PRED_F64) return t.p_off[i + 1] - t.p_off[i];
    const int n = t.num[i];
    return n < 0 ? 0 : n < t.max_people ? n : t.max_people;
}
HH_HD bool pose_fallback(const PoseTables &t, int i) { return t.form == HH_POSE_PRED_DECODE && t.flags && (t.flags[i] & HH_DECODE_FALLBACK); }

// Coordinate c (0 = x, 1 = y) of joint k of prediction p of image i, as the rule reads it.
HH_HD double pose_pred_coord(const PoseTables &t, int i, int p, int k, int c, bool fallback)
{
    if (t.form == HH_POSE_PRED_F64) return t.p_xy[((size_t)(t.p_off[i] + p) * t.K + k) * 2 + c];
    const float *j = t.joints + (size_t)i * t.image_stride + (size_t)p * t.person_stride + (size_t)k * t.joint_stride;
    const double *M = t.inv_affine + (size_t)i * 6 + 3 * c;
    const double x = (double)j[0], y = (double)j[1];
    const double u = M[0] * x + M[1] * y + M[2] * 1.0;
    return fallback ? u : (double)(float)u;
}
HH_HD double pose_pred_score(const PoseTables &t, int i, int p, bool fallback)
{
    if (t.form == HH_POSE_PRED_F64) return t.p_score[t.p_off[i] + p];
    if (!fallback) return (double)t.scores[(size_t)i * t.score_stride + p];
    double s = 0.0;
    for (int k = 0; k < t.K; ++k) s += 0.01;
    return s / (double)t.K;
}

// The position of prediction p in the walk (ascending score, equal scores by ascending index); scores are finite.
HH_HD int pose_rank(const double *score, int P, int p)
{
    int r = 0;
    for (int q = 0; q < P; ++q) r += (score[q] < score[p] || (score[q] == score[p] && q < p)) ? 1 : 0;
    return r;
}

HH_HD int pose_visible(const double *xyv, int K)
{
    int n = 0;
    for (int k = 0; k < K; ++k) n += xyv[3 * k + 2] > 0.0 ? 1 : 0;
    return n;
}

// val = 1 / D of one (prediction, target) pair: pxy [K,2], xyv [K,3], n = pose_visible(xyv) > 0.
HH_HD double pose_match_val(const double *pxy, const double *xyv, int K, int n)
{
    double sum = 0.0;
    for (int k = 0; k < K; ++k) {
        if (!(xyv[3 * k + 2] > 0.0)) continue;
        const double dx = pxy[2 * k] - xyv[3 * k], dy = pxy[2 * k + 1] - xyv[3 * k + 1];
        sum += dx * dx + dy * dy;
    }
    return 1.0 / (sum / (double)n);
}

// "a comes before b" for the strict-greater walk: the final holder is the first position in walk order that reaches the largest val, so
// a reduction over (val, rank) in any order finds it.  A NaN val never holds (it is never greater).
HH_HD bool pose_better(double va, int ra, double vb, int rb) { return va > vb || (va == vb && ra < rb); }

// The per-joint term of target joint k against the matched prediction: exp(-e_k) or the hit, -1 for an unlabelled joint.
HH_HD double pose_term(const PoseTables &t, const double *pxy, const double *xyv, double area, double head, int k)
{
    if (!(xyv[3 * k + 2] > 0.0)) return -1.0;
    if (t.metric == HH_POSE_METRIC_OKS) {
        const double dx = pxy[2 * k] - xyv[3 * k], dy = pxy[2 * k + 1] - xyv[3 * k + 1];
        const double e = (dx * dx + dy * dy) / ((2.0 * t.vars[k]) * area);
        return exp(-e);
    }
    const double dx = pxy[2 * k] / head - xyv[3 * k] / head, dy = pxy[2 * k + 1] / head - xyv[3 * k + 1] / head;
    return sqrt(dx * dx + dy * dy) < t.alpha ? 1.0 : 0.0;
}

// obj[t] from the K terms, ascending k.
HH_HD double pose_object(const double *term, int K, int n)
{
    double sum = 0.0;
    for (int k = 0; k < K; ++k)
        if (term[k] >= 0.0) sum += term[k];
    return sum / (double)n;
}

// The image value from its T object values, ascending t.
HH_HD double pose_image_value(const double *obj, int T, int metric)
{
    double sum = 0.0;
    int n = 0;
    for (int j = 0; j < T; ++j) {
        if (metric == HH_POSE_METRIC_OKS) sum += rint(obj[j] * 1000.0) / 1000.0, ++n;
        else if (obj[j] != -1.0) sum += obj[j], ++n;
    }
    return n ? sum / (double)n : -1.0;
}

// One image on the host, what a workgroup does; the walk is done literally (sorted order, strict greater), which the kernel's reduction
// has to equal.  `pxy`: P * K * 2 doubles, `score`: P doubles, `term`: K doubles of scratch.
inline void pose_image_host(const PoseTables &t, int i, double *pxy, double *score, double *term, double *value, double *obj, double *kpt, int32_t *match,
                            int32_t *status)
{
    const int K = t.K, P = pose_num_preds(t, i), t0 = t.t_off[i], T = t.t_off[i + 1] - t0;
    const bool fb = pose_fallback(t, i);
    int st = P == 0 && T > 0 ? HH_POSE_NO_PRED : 0;
    for (int p = 0; p < P; ++p) {
        score[p] = pose_pred_score(t, i, p, fb);
        if (!pose_finite(score[p])) st |= HH_POSE_NONFINITE;
        for (int e = 0; e < K * 2; ++e) {
            pxy[(size_t)p * K * 2 + e] = pose_pred_coord(t, i, p, e / 2, e % 2, fb);
            if (!pose_finite(pxy[(size_t)p * K * 2 + e])) st |= HH_POSE_NONFINITE;
        }
    }
    status[i] = st;
    if (st) {
        value[i] = pose_nan();
        for (int j = t0; j < t0 + T; ++j) {
            obj[j] = pose_nan();
            match[j] = -1;
            for (int k = 0; k < K; ++k) kpt[(size_t)j * K + k] = pose_nan();
        }
        return;
    }
    int order[HH_POSE_MAX_P];
    for (int p = 0; p < P; ++p) order[pose_rank(score, P, p)] = p;
    for (int j = 0; j < T; ++j) {
        const double *xyv = t.t_xyv + (size_t)(t0 + j) * K * 3;
        const int n = pose_visible(xyv, K);
        double best = -INFINITY;
        int m = -1;
        for (int r = 0; r < P; ++r) {
            const double v = pose_match_val(pxy + (size_t)order[r] * K * 2, xyv, K, n);
            if (v > best) best = v, m = order[r];
        }
        match[t0 + j] = m;  // (P > 0 and everything finite: the first prediction's val > -inf, so m >= 0)
        const double head = t.t_head[t0 + j];
        if (t.metric == HH_POSE_METRIC_PCKH && head == 0.0) {
            obj[t0 + j] = -1.0;
            for (int k = 0; k < K; ++k) kpt[(size_t)(t0 + j) * K + k] = -1.0;
            continue;
        }
        for (int k = 0; k < K; ++k) kpt[(size_t)(t0 + j) * K + k] = term[k] = pose_term(t, pxy + (size_t)m * K * 2, xyv, t.t_area[t0 + j], head, k);
        obj[t0 + j] = pose_object(term, K, n);
    }
    value[i] = pose_image_value(obj + t0, T, t.metric);
}

// cv2.contourArea of the int32-truncated polygon as an exact int64 shoelace (|coordinates| <= 2^30, n < 2^31: every product is below 2^60;
// the sum is taken in __int128 so that no polygon can overflow it).
inline int pose_polygon_area(const double *xy, int n, double *area)
{
    if (n < 0 || (n > 0 && !xy) || !area) return 1;
    for (int j = 0; j < 2 * n; ++j)
        if (!pose_finite(xy[j]) || fabs(xy[j]) > 1073741824.0) return 1;
    *area = 0.0;
    if (n < 3) return 0;
    __int128 a = 0;
    int64_t xp = (int64_t)xy[2 * (n - 1)], yp = (int64_t)xy[2 * (n - 1) + 1];
    for (int j = 0; j < n; ++j) {
        const int64_t x = (int64_t)xy[2 * j], y = (int64_t)xy[2 * j + 1];
        a += (__int128)xp * y - (__int128)yp * x;
        xp = x;
        yp = y;
    }
    if (a < 0) a = -a;
    *area = (double)a * 0.5;
    return 0;
}

// What the entry points refuse, on host copies of the tables; returns nullptr when accepted, otherwise a message (in `msg`, >= 192 bytes,
// where it names an image).  Reads inv_affine, p_off (by form), t_off, t_xyv, t_area, t_head, vars, alpha; never a prediction.
inline const char *pose_check(const PoseTables &t, char *msg, size_t msg_len)
{
    if (t.form != HH_POSE_PRED_DECODE && t.form != HH_POSE_PRED_F64) return "form is neither HH_POSE_PRED_DECODE nor HH_POSE_PRED_F64";
    if (t.metric != HH_POSE_METRIC_OKS && t.metric != HH_POSE_METRIC_PCKH) return "metric is neither HH_POSE_METRIC_OKS nor HH_POSE_METRIC_PCKH";
    if (t.B < 0 || t.B > (1 << 24)) return "B outside 0..2^24";
    if (t.K < 1 || t.K > HH_POSE_MAX_K) return "K outside 1..HH_POSE_MAX_K (64)";
    if (!t.t_off || !t.t_xyv || !t.t_area || !t.t_head) return "null pointer";
    if (!pose_finite(t.alpha)) return "alpha is not finite";
    for (int k = 0; k < t.K; ++k)
        if (!(t.vars[k] > 0.0) || !pose_finite(t.vars[k])) return "vars must be finite and > 0";
    if (t.form == HH_POSE_PRED_DECODE) {
        if (!t.inv_affine) return "null pointer";
        if (t.max_people < 1 || t.max_people > HH_POSE_MAX_P) return "max_people outside 1..HH_POSE_MAX_P (64): refused, not capped";
        if (t.image_stride < 0 || t.person_stride < 0 || t.joint_stride < 0 || t.score_stride < 0) return "negative stride";
        for (int i = 0; i < t.B; ++i)
            for (int e = 0; e < 6; ++e)
                if (!pose_finite(t.inv_affine[(size_t)i * 6 + e])) {
                    snprintf(msg, msg_len, "image %d: non-finite inverse matrix", i);
                    return msg;
                }
    } else {
        if (!t.p_off) return "null pointer";
        if (t.p_off[0] != 0) return "p_off does not start at 0";
        for (int i = 0; i < t.B; ++i) {
            const long long P = (long long)t.p_off[i + 1] - t.p_off[i];
            if (P < 0) {
                snprintf(msg, msg_len, "image %d: p_off decreases", i);
                return msg;
            }
            if (P > HH_POSE_MAX_P) {
                snprintf(msg, msg_len, "image %d has %lld predictions, over HH_POSE_MAX_P (64): refused, not capped", i, P);
                return msg;
            }
        }
    }
    if (t.t_off[0] != 0) return "t_off does not start at 0";
    for (int i = 0; i < t.B; ++i) {
        const long long T = (long long)t.t_off[i + 1] - t.t_off[i];
        if (T < 0) {
            snprintf(msg, msg_len, "image %d: t_off decreases", i);
            return msg;
        }
        if (T > HH_POSE_MAX_T) {
            snprintf(msg, msg_len, "image %d has %lld targets, over HH_POSE_MAX_T (128): refused, not capped", i, T);
            return msg;
        }
        for (int j = t.t_off[i]; j < t.t_off[i + 1]; ++j) {
            const double *xyv = t.t_xyv + (size_t)j * t.K * 3;
            for (int e = 0; e < t.K * 3; ++e)
                if (!pose_finite(xyv[e])) {
                    snprintf(msg, msg_len, "image %d: target %d has a non-finite value", i, j - t.t_off[i]);
                    return msg;
                }
            if (pose_visible(xyv, t.K) == 0) {
                snprintf(msg, msg_len, "image %d: target %d has no labelled joint", i, j - t.t_off[i]);
                return msg;
            }
            if (!(t.t_area[j] > 0.0) || !pose_finite(t.t_area[j])) {
                snprintf(msg, msg_len, "image %d: target %d: area must be finite and > 0", i, j - t.t_off[i]);
                return msg;
            }
            if (!(t.t_head[j] >= 0.0) || !pose_finite(t.t_head[j])) {
                snprintf(msg, msg_len, "image %d: target %d: head size must be finite and >= 0", i, j - t.t_off[i]);
                return msg;
            }
        }
    }
    return nullptr;
}
#endif
