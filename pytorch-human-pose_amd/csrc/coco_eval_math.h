// COCO keypoint scoring (keypoints/coco_eval.py: _oks = pycocotools' computeOks, _evaluate_img = evaluateImg), kept apart from the kernel
// so that the same text also compiles for the host (hh_coco_evaluate_host, tools/coco_eval_host_check.cpp): the packed tables, the OKS of
// one (detection, ground truth) pair, the matching walk of one (image, area range, threshold), one image in plain loops, the validation.
// Compile with -ffp-contract=off: every fp64 operation of the OKS rounds on its own, so the exponent e is bit-identical to numpy's; only
// exp() and the order of the sum over joints may differ from the host evaluator.  The walk does no floating-point arithmetic, only
// comparisons, so given the same OKS matrix it is exact.
#ifndef HH_COCO_EVAL_MATH_H
#define HH_COCO_EVAL_MATH_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/hhrnet.h"
#include "host_dev.h"

// The limits are HH_COCO_* of include/hhrnet.h.  One workgroup owns one image: its D x G OKS values live in LDS (32 KB of fp64 at the limits),
// one lane walks one (area range, threshold) with the "ground truth taken" set as two 64-bit words, so A * T <= 64 = one wave.
enum { COCO_THREADS = 256 };
static_assert(HH_COCO_MAX_A * HH_COCO_MAX_T <= 64 && HH_COCO_MAX_GT == 128, "one wave of walks, two words of ground truths");

using CocoTables = hh_coco_tables;
static_assert(sizeof(hh_coco_tables) == 136, "ABI 3");

// np.max((0, a)) of one element: NaN stays NaN.
HH_HD double coco_pos(double a) { return a <= 0.0 ? 0.0 : a; }

// computeOks for one pair, in the operation order of COCOKeypointsEval._oks.  xy: the detection's K x 2; xyv: the ground truth's K x 3.
HH_HD double coco_oks_pair(const double *xy, const double *xyv, const double *bbox, double area, const double *vars, int K)
{
    int k1 = 0;
    for (int k = 0; k < K; ++k) k1 += xyv[3 * k + 2] > 0.0 ? 1 : 0;
    const double x0 = bbox[0] - bbox[2], x1 = bbox[0] + bbox[2] * 2.0;
    const double y0 = bbox[1] - bbox[3], y1 = bbox[1] + bbox[3] * 2.0;
    const double den = area + 2.220446049250313e-16;  // np.spacing(1) = 2^-52
    double sum = 0.0;
    for (int k = 0; k < K; ++k) {
        const double xd = xy[2 * k], yd = xy[2 * k + 1];
        double dx, dy;
        if (k1 > 0) {
            if (!(xyv[3 * k + 2] > 0.0)) continue;  // e[vg > 0]
            dx = xd - xyv[3 * k];
            dy = yd - xyv[3 * k + 1];
        } else {  // no labelled joint: distance to the doubled box
            dx = coco_pos(x0 - xd) + coco_pos(xd - x1);
            dy = coco_pos(y0 - yd) + coco_pos(yd - y1);
        }
        const double e = (dx * dx + dy * dy) / vars[k] / den / 2.0;
        sum += exp(-e);
    }
    return sum / (double)(k1 > 0 ? k1 : K);
}

// The ground truths of one image for one area range as two bit sets over the packed (original) order: ignored, and crowd.
struct CocoGtSets { uint64_t ign[2], crowd[2]; };
HH_HD bool coco_gt_ignored(double area, int flags, double lo, double hi) { return (flags & HH_COCO_GT_IGNORE) || area < lo || area > hi; }
HH_HD CocoGtSets coco_gt_sets(const double *gt_area, const uint8_t *gt_flags, int G, double lo, double hi)
{
    CocoGtSets s;
    s.ign[0] = s.ign[1] = s.crowd[0] = s.crowd[1] = 0;
#if defined(__clang__)
#pragma unroll
#endif
    for (int w = 0; w < 2; ++w)
        for (int b = 0; b < 64 && w * 64 + b < G; ++b) {
            const int g = w * 64 + b;
            if (coco_gt_ignored(gt_area[g], gt_flags[g], lo, hi)) s.ign[w] |= 1ull << b;
            if (gt_flags[g] & HH_COCO_GT_CROWD) s.crowd[w] |= 1ull << b;
        }
    return s;
}
// gt_ignore of the image's G ground truths for one area, in packed order: writes out[0 .. G - 1].
HH_HD void coco_store_gt_ignore(const CocoGtSets &s, int G, uint8_t *out)
{
#if defined(__clang__)
#pragma unroll
#endif
    for (int w = 0; w < 2; ++w)
        for (int b = 0; b < 64 && w * 64 + b < G; ++b) out[w * 64 + b] = (uint8_t)((s.ign[w] >> b) & 1);
}

// evaluateImg for one (area range, threshold) of one image: oks is the image's D x G matrix, row-major, in the packed orders.  The
// reference walks the ground truths in the stable partition "not ignored first"; that order is pass 0 (not ignored) followed by pass 1
// (ignored), each in packed order, so the permutation is never materialised.  dt_match[d] = gt_base + g + 1 of the matched ground truth
// (its row in the packed table + 1) or 0; dt_ignore[d] = the matched ground truth's flag, or "the detection's area is outside the range"
// when unmatched.  Writes exactly dt_match[0 .. D - 1] and dt_ignore[0 .. D - 1]; reads oks[0 .. D * G - 1], dt_area[0 .. D - 1].
HH_HD void coco_match_walk(const double *oks, int D, int G, const CocoGtSets &s, double t, const double *dt_area, double lo, double hi, int gt_base,
                            int32_t *dt_match, uint8_t *dt_ignore)
{
    const double start = t < 1 - 1e-10 ? t : 1 - 1e-10;  // min([t, 1 - 1e-10])
    uint64_t taken[2] = {0, 0};
    for (int d = 0; d < D; ++d) {
        double iou = start;
        int m = -1;
        bool m_ign = false, stop = false;
#if defined(__clang__)
#pragma unroll
#endif
        for (int pass = 0; pass < 2; ++pass)
#if defined(__clang__)
#pragma unroll
#endif
            for (int w = 0; w < 2; ++w) {
                if (stop) continue;
                for (int b = 0; b < 64 && w * 64 + b < G; ++b) {
                    const uint64_t bit = 1ull << b;
                    const bool gi = (s.ign[w] & bit) != 0;
                    if (gi != (pass == 1)) continue;                         // (not this pass's half of the partition)
                    if ((taken[w] & bit) && !(s.crowd[w] & bit)) continue;   // already matched and not a crowd
                    if (m > -1 && !m_ign && gi) { stop = true; break; }      // the best so far is a real one and the ignored ones begin
                    const double v = oks[(size_t)d * G + w * 64 + b];
                    if (v < iou) continue;                                   // (an equal OKS on a later ground truth takes the match over)
                    iou = v;
                    m = w * 64 + b;
                    m_ign = gi;
                }
            }
        if (m < 0) {
            dt_match[d] = 0;
            dt_ignore[d] = (dt_area[d] < lo || dt_area[d] > hi) ? 1 : 0;
        } else {
            dt_match[d] = gt_base + m + 1;
            dt_ignore[d] = m_ign ? 1 : 0;
            if (m < 64) taken[0] |= 1ull << m;  // (no dynamic index: the two words stay in registers)
            else taken[1] |= 1ull << (m - 64);
        }
    }
}

// What the hh_coco_* entry points refuse, on the caller's host copy of the tables; returns nullptr when accepted, otherwise a message in
// `msg` (>= 160 bytes).  Reads dt_off, gt_off, oks_off, dt_area, gt_area, vars, area_rng and thr; never the coordinates.
inline const char *coco_check(const CocoTables *t, char *msg, size_t msg_len);

// One image on the host, what a workgroup does.  oks_in: read the image's matrix from it (match only); otherwise compute it into `scratch`
// (HH_COCO_MAX_DET * HH_COCO_MAX_GT doubles) and, if oks_out, store it there.  `match`: run the walks and write the three outputs.
inline void coco_image_host(const CocoTables &t, int i, const double *oks_in, double *oks_out, double *scratch, bool match, int32_t *dt_match,
                            uint8_t *dt_ignore, uint8_t *gt_ignore)
{
    const int d0 = t.dt_off[i], D = t.dt_off[i + 1] - d0, g0 = t.gt_off[i], G = t.gt_off[i + 1] - g0;
    const double *oks = oks_in ? oks_in + t.oks_off[i] : scratch;
    if (!oks_in)
        for (int d = 0; d < D; ++d)
            for (int g = 0; g < G; ++g) {
                const double v = coco_oks_pair(t.dt_xy + (size_t)(d0 + d) * t.K * 2, t.gt_xyv + (size_t)(g0 + g) * t.K * 3, t.gt_bbox + (size_t)(g0 + g) * 4,
                                               t.gt_area[g0 + g], t.vars, t.K);
                scratch[(size_t)d * G + g] = v;
                if (oks_out) oks_out[t.oks_off[i] + (size_t)d * G + g] = v;
            }
    if (!match) return;
    for (int a = 0; a < t.A; ++a) {
        const double lo = t.area_rng[2 * a], hi = t.area_rng[2 * a + 1];
        const CocoGtSets s = coco_gt_sets(t.gt_area + g0, t.gt_flags + g0, G, lo, hi);
        coco_store_gt_ignore(s, G, gt_ignore + (size_t)a * t.M + g0);
        for (int k = 0; k < t.T; ++k) {
            const size_t o = ((size_t)a * t.T + k) * t.N + d0;
            coco_match_walk(oks, D, G, s, t.thr[k], t.dt_area + d0, lo, hi, g0, dt_match + o, dt_ignore + o);
        }
    }
}

#include <stdio.h>
inline const char *coco_check(const CocoTables *t, char *msg, size_t msg_len)
{
    if (!t) return "null pointer";
    if (!t->dt_off || !t->gt_off || !t->oks_off || !t->dt_xy || !t->dt_score || !t->dt_area || !t->gt_xyv || !t->gt_area || !t->gt_bbox || !t->gt_flags ||
        !t->vars || !t->area_rng || !t->thr)
        return "null pointer";
    if (t->I < 0 || t->I > (1 << 24) || t->N < 0 || t->M < 0) return "image, detection or ground-truth count out of range";
    if (t->K < 1 || t->K > HH_COCO_MAX_K) return "K outside 1..64";
    if (t->T < 1 || t->T > HH_COCO_MAX_T) return "T outside 1..HH_COCO_MAX_T (16)";
    if (t->A < 1 || t->A > HH_COCO_MAX_A) return "A outside 1..HH_COCO_MAX_A (4)";
    if ((long long)t->N * t->A * t->T > (1ll << 31) - 1 || (long long)t->M * t->A > (1ll << 31) - 1) return "output beyond 2^31 elements";
    if (t->dt_off[0] != 0 || t->gt_off[0] != 0 || t->oks_off[0] != 0) return "offsets do not start at 0";
    for (int i = 0; i < t->I; ++i) {
        const long long D = (long long)t->dt_off[i + 1] - t->dt_off[i], G = (long long)t->gt_off[i + 1] - t->gt_off[i];
        if (D < 0 || G < 0 || t->dt_off[i + 1] > t->N || t->gt_off[i + 1] > t->M) {
            snprintf(msg, msg_len, "non-monotone or out-of-range offsets at image %d", i);
            return msg;
        }
        if (D > HH_COCO_MAX_DET) {
            snprintf(msg, msg_len, "image %d has %lld detections, over HH_COCO_MAX_DET (32)", i, D);
            return msg;
        }
        if (G > HH_COCO_MAX_GT) {
            snprintf(msg, msg_len, "image %d has %lld ground truths, over HH_COCO_MAX_GT (128)", i, G);
            return msg;
        }
    }
    if (t->dt_off[t->I] != t->N || t->gt_off[t->I] != t->M) return "offsets do not end at N and M";
    for (int i = 0; i < t->I; ++i)
        if (t->oks_off[i + 1] - t->oks_off[i] != (long long)(t->dt_off[i + 1] - t->dt_off[i]) * (t->gt_off[i + 1] - t->gt_off[i])) {
            snprintf(msg, msg_len, "oks_off does not advance by D * G at image %d", i);
            return msg;
        }
    for (int k = 0; k < t->K; ++k)
        if (!(t->vars[k] > 0.0) || !isfinite(t->vars[k])) return "vars must be finite and > 0";
    for (int n = 0; n < t->N; ++n)
        if (!isfinite(t->dt_area[n])) return "non-finite detection area";
    for (int m = 0; m < t->M; ++m)
        if (!isfinite(t->gt_area[m])) return "non-finite ground-truth area";
    for (int a = 0; a < 2 * t->A; ++a)
        if (t->area_rng[a] != t->area_rng[a]) return "NaN in area_rng";
    for (int k = 0; k < t->T; ++k)
        if (t->thr[k] != t->thr[k]) return "NaN in thr";
    return nullptr;
}
#endif
