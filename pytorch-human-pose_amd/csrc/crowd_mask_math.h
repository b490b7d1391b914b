// The arithmetic of the crowd masks (crowd_mask.hip; the rule is stated at hh_crowd_polygon_toggles / hh_crowd_masks_u8_batch in
// include/hhrnet.h), kept apart from the kernel so that the same text also compiles for the host (hh_crowd_polygon_toggles,
// hh_debug_crowd_masks_host, tools/crowd_mask_host_check.cpp): the descriptors, the per-pixel predicate as an upper-bound search, a
// tile column's coverage as a row bitmask, one mask walked tile by tile in plain loops, the validation, and -- host only -- the
// polygon walk with its cancel step.  Compile with -ffp-contract=off: every double operation of the walk rounds on its own.
#ifndef HH_CROWD_MASK_MATH_H
#define HH_CROWD_MASK_MATH_H
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../include/hhrnet.h"
#include "host_dev.h"

// The launch geometry, reported by hh_crowd_mask_config: a workgroup of CROWD_THREADS threads owns a tile of CROWD_TW columns x
// CROWD_TH rows; in the first phase a lane owns one column of the tile and forms its CROWD_TH coverage bits in one uint32 (row r of
// the tile = bit r), in the second phase a lane owns four adjacent bytes of a row.  The toggles are read where they lie: there is no
// per-chunk toggle capacity (reported as 0).
enum { CROWD_TW = 256, CROWD_TH = 32, CROWD_THREADS = 256, CROWD_MAX_SIDE = 16384 };
static_assert(CROWD_TW == CROWD_THREADS && CROWD_TH == 32 && CROWD_TW % 4 == 0, "one lane per tile column, one bit per tile row");

using CrowdMaskDesc = hh_crowd_mask_desc;
using CrowdSegDesc = hh_crowd_seg_desc;
static_assert(sizeof(hh_crowd_mask_desc) == 24 && sizeof(hh_crowd_seg_desc) == 24, "ABI 3");

// The number of toggles <= idx (an upper-bound search): pixel idx is covered by the segment iff it is odd.
HH_HD uint32_t crowd_upper_bound(const uint32_t *t, uint32_t n, uint32_t idx)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (t[mid] <= idx) lo = mid + 1; else hi = mid;
    }
    return lo;
}
HH_HD bool crowd_covered(const uint32_t *t, uint32_t n, uint32_t idx) { return crowd_upper_bound(t, n, idx) & 1; }

// Coverage of the pixels idx0 .. idx0 + rows - 1 (1 <= rows <= 32, all in one image column) as bits 0 .. rows - 1: one search for the
// top pixel, then a cursor down the sorted list; a toggle at idx0 + r flips every bit from r on.  Bits from `rows` on are unspecified.
HH_HD uint32_t crowd_column_bits(const uint32_t *t, uint32_t n, uint32_t idx0, int rows)
{
    uint32_t c = crowd_upper_bound(t, n, idx0);
    uint32_t bits = (c & 1) ? ~0u : 0u;
    const uint32_t last = idx0 + (uint32_t)rows - 1;  // < h * w <= 2^28
    while (c < n && t[c] <= last) {
        bits ^= ~0u << (t[c] - idx0);                 // t[c] - idx0 in 1 .. 31
        ++c;
    }
    return bits;
}

// Column x of one mask, rows ty0 .. ty0 + rows - 1: the union over the mask's segments, each culled by its column range.
HH_HD uint32_t crowd_lane_bits(const unsigned char *base, const CrowdSegDesc *segs, const CrowdMaskDesc &d, int x, int ty0, int rows)
{
    uint32_t bits = 0;
    for (int s = d.seg_first; s < d.seg_first + d.seg_count; ++s) {
        const CrowdSegDesc &sg = segs[s];
        if (x < sg.col_first || x > sg.col_last) continue;
        bits |= crowd_column_bits(reinterpret_cast<const uint32_t *>(base + sg.toggle_offset), (uint32_t)sg.count, (uint32_t)x * (uint32_t)d.h + (uint32_t)ty0, rows);
    }
    return bits;
}

// One mask on the host, in the kernel's own walk: tile by tile, a row bitmask per tile column, then the tile's bytes row by row.
// `mask` is the h * w output (the descriptor's mask_offset is not applied); `base` is what the toggle offsets count from.
inline void crowd_mask_host(unsigned char *mask, const CrowdMaskDesc &d, const CrowdSegDesc *segs, const unsigned char *base)
{
    for (int ty0 = 0; ty0 < d.h; ty0 += CROWD_TH)
        for (int tx0 = 0; tx0 < d.w; tx0 += CROWD_TW) {
            const int rows = d.h - ty0 < CROWD_TH ? d.h - ty0 : CROWD_TH, cols = d.w - tx0 < CROWD_TW ? d.w - tx0 : CROWD_TW;
            uint32_t bits[CROWD_TW];
            for (int lane = 0; lane < cols; ++lane) bits[lane] = crowd_lane_bits(base, segs, d, tx0 + lane, ty0, rows);
            for (int r = 0; r < rows; ++r)
                for (int c = 0; c < cols; ++c) mask[(size_t)(ty0 + r) * d.w + tx0 + c] = (bits[c] >> r & 1) ? 0 : 255;
        }
}

// What hh_crowd_masks_u8_batch refuses for one mask, on the caller's host copies; nullptr = accepted.  `host_base` holds the staged
// bytes (the toggles at the offsets the device sees them at).
inline const char *crowd_check_mask(const CrowdMaskDesc &d, const CrowdSegDesc *segs, long long num_segs, const unsigned char *host_base)
{
    if (d.h < 1 || d.w < 1 || d.h > CROWD_MAX_SIDE || d.w > CROWD_MAX_SIDE) return "mask size outside 1..16384";
    if (d.mask_offset < 0) return "negative mask offset";
    if (d.seg_count < 0 || d.seg_first < 0 || (long long)d.seg_first + d.seg_count > num_segs) return "segment range outside the table";
    const uint32_t area = (uint32_t)d.h * (uint32_t)d.w;
    for (int s = d.seg_first; s < d.seg_first + d.seg_count; ++s) {
        const CrowdSegDesc &sg = segs[s];
        if (sg.toggle_offset < 0 || sg.toggle_offset % 4) return "toggle offset negative or not a multiple of 4";
        if (sg.count < 0) return "negative toggle count";
        if (sg.col_first < 0 || sg.col_last >= d.w || sg.col_first > sg.col_last) return "column range outside the image";
        const uint32_t *t = reinterpret_cast<const uint32_t *>(host_base + sg.toggle_offset);
        for (int i = 0; i < sg.count; ++i) {
            if (t[i] > area) return "toggle above h*w";
            if (i && t[i] <= t[i - 1]) return "toggles not strictly increasing";
        }
        // the range must hold every covered column: the first toggle's, and the column before the last toggle (an odd count covers
        // through the last pixel), else the cull would change the result
        if (sg.count > 0 && t[0] < area) {
            const int first = (int)(t[0] / (uint32_t)d.h), last = (sg.count & 1) ? d.w - 1 : (int)((t[sg.count - 1] - 1) / (uint32_t)d.h);
            if (sg.col_first > first || sg.col_last < last) return "column range does not hold the segment";
        }
    }
    return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------- host only
// What hh_crowd_polygon_toggles refuses; nullptr = accepted.
inline const char *crowd_polygon_check(const double *xy, int k, int h, int w)
{
    if (k < 3) return "a polygon needs at least 3 vertices";
    if (h < 1 || w < 1 || h > CROWD_MAX_SIDE || w > CROWD_MAX_SIDE) return "image size outside 1..16384";
    for (int i = 0; i < 2 * k; ++i) {
        if (!(xy[i] - xy[i] == 0.0)) return "coordinate not finite";
        const double v = 5 * xy[i] + 0.5;
        if (!(v > -2147483649.0 && v < 2147483648.0)) return "five-fold coordinate outside the int range";
    }
    return nullptr;
}

static inline int crowd_snap(double v) { return (int)(5 * v + 0.5); }

// An upper bound of the toggle count, from the vertices alone: positions are emitted only where u changes onto a column centre
// (every fifth u), so an edge of dx grid steps emits at most dx / 5 + 2, and never more than two per image column.
inline long long crowd_polygon_bound(const double *xy, int k, int w)
{
    long long total = 0;
    for (int j = 0; j < k; ++j) {
        const int jn = j + 1 < k ? j + 1 : 0;
        const long long dx = llabs((long long)crowd_snap(xy[2 * jn]) - (long long)crowd_snap(xy[2 * j]));
        total += std::min<long long>(dx / 5 + 2, 2LL * w);
    }
    return total;
}

// Step 4: sort, drop values of even multiplicity, keep values of odd multiplicity once.
inline void crowd_cancel(std::vector<uint32_t> &p)
{
    std::sort(p.begin(), p.end());
    size_t n = 0;
    for (size_t i = 0; i < p.size();) {
        size_t j = i;
        while (j < p.size() && p[j] == p[i]) ++j;
        if ((j - i) & 1) p[n++] = p[i];
        i = j;
    }
    p.resize(n);
}

// Steps 1-3 (the caller has run crowd_polygon_check): the emitted positions appended to `out`, in walk order.  The points are not
// stored: only the previous one is needed.
inline void crowd_polygon_walk(const double *xy, int k, int h, int w, std::vector<uint32_t> &out)
{
    std::vector<int> X((size_t)k + 1), Y((size_t)k + 1);
    for (int j = 0; j < k; ++j) X[j] = crowd_snap(xy[2 * j]), Y[j] = crowd_snap(xy[2 * j + 1]);
    X[k] = X[0], Y[k] = Y[0];
    bool have = false;
    int pu = 0, pv = 0;
    auto point = [&](int u, int v) {
        if (have && u != pu) {
            double xd = (double)(u < pu ? u : u - 1);
            xd = (xd + 0.5) / 5 - 0.5;
            if (floor(xd) == xd && xd >= 0 && xd <= w - 1) {
                double yd = (double)(v < pv ? v : pv);
                yd = (yd + 0.5) / 5 - 0.5;
                if (yd < 0) yd = 0; else if (yd > h) yd = h;
                yd = ceil(yd);
                out.push_back((uint32_t)((int)xd * h + (int)yd));
            }
        }
        pu = u, pv = v, have = true;
    };
    for (int j = 0; j < k; ++j) {
        const long long dx = llabs((long long)X[j + 1] - X[j]), dy = llabs((long long)Y[j + 1] - Y[j]);
        const bool flipped = (dx >= dy && X[j] > X[j + 1]) || (dx < dy && Y[j] > Y[j + 1]);
        const long long xs = flipped ? X[j + 1] : X[j], ys = flipped ? Y[j + 1] : Y[j];
        const long long xe = flipped ? X[j] : X[j + 1], ye = flipped ? Y[j] : Y[j + 1];
        if (dx == 0 && dy == 0) {
            point(X[j], Y[j]);
        } else if (dx >= dy) {
            const double s = (double)(ye - ys) / (double)dx;
            for (long long d = 0; d <= dx; ++d) {
                const long long t = flipped ? dx - d : d;
                point((int)(xs + t), (int)((double)ys + s * (double)t + 0.5));
            }
        } else {
            const double s = (double)(xe - xs) / (double)dy;
            for (long long d = 0; d <= dy; ++d) {
                const long long t = flipped ? dy - d : d;
                point((int)((double)xs + s * (double)t + 0.5), (int)(ys + t));
            }
        }
    }
}
#endif
