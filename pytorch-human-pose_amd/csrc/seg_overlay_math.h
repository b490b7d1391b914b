// The arithmetic of the segmentation overlay (seg_overlay.hip; the rule is stated at hh_seg_overlay_u8_batch in include/hhrnet.h), kept
// apart from the kernel so that the same text also compiles for the host (hh_debug_seg_overlay_host, tools/seg_overlay_host_check.cpp):
// the shape rows, the tile cull, the rows of one image column that a shape covers as a bitmask (the fill through crowd_mask_math.h's
// toggle predicate, the line through its exact int64 rule), the blend (render_math.h's), one frame walked tile by tile in plain loops,
// and the validation.  Compile with -ffp-contract=off: every fp32 operation of the blend rounds on its own.
#ifndef HH_SEG_OVERLAY_MATH_H
#define HH_SEG_OVERLAY_MATH_H
#include "crowd_mask_math.h"
#include "render_math.h"

// The launch geometry, reported by hh_seg_overlay_config: a workgroup of SEG_THREADS threads owns a tile of SEG_TH rows x SEG_TW columns.
// In the first phase a thread owns SEG_ROWS rows of one tile column (thread t: column t % SEG_TW, rows t / SEG_TW * SEG_ROWS on) and
// keeps their overlay colours in registers while the frame's shapes, culled to the tile SEG_CHUNK at a time, pass in draw order; in
// the second phase a thread owns SEG_PX horizontally adjacent pixels of a row.
enum { SEG_TH = 32, SEG_TW = 128, SEG_ROWS = 16, SEG_PX = 4, SEG_THREADS = SEG_TW * (SEG_TH / SEG_ROWS), SEG_CHUNK = SEG_THREADS };
enum { SEG_PITCH = SEG_TW + SEG_PX, SEG_COVERED = 1 << 24, SEG_MAX_COORD = 1 << 23 };
static_assert(SEG_THREADS == 256 && SEG_TH % SEG_ROWS == 0 && SEG_ROWS <= 32 && SEG_TW % SEG_PX == 0 && SEG_PX == 4, "a row bitmask per thread, whole pixel groups per tile row");
static_assert(SEG_TW / SEG_PX == 32 && SEG_THREADS / 32 <= SEG_TH, "second phase: a half-wave per tile row");

using SegDesc = hh_seg_desc;
struct SegShape { int32_t v[HH_SEG_SHAPE_INTS]; };  // {kind, colour, a, b, c, d, 0, 0}
static_assert(sizeof(SegShape) == 32 && sizeof(hh_seg_desc) == 48, "ABI 3");
// What the kernel keeps of a shape that survived the cull.
struct SegItem { int32_t kind, colour, a, b, c, d; };

HH_HD long long seg_floor_div(long long n, long long d)  // d > 0; toward minus infinity
{
    const long long q = n / d;
    return (n % d != 0 && n < 0) ? q - 1 : q;
}
HH_HD long long seg_ceil_div(long long n, long long d) { return -seg_floor_div(-n, d); }  // d > 0

// Does the shape meet the tile [tx0, tx1] x [ty0, ty1] (inclusive, inside the frame)?  A fill is culled by its column range alone.
HH_HD bool seg_meets(const SegShape &s, int tx0, int ty0, int tx1, int ty1)
{
    if (s.v[0] == HH_SEG_FILL) return s.v[3] > 0 && s.v[4] <= tx1 && s.v[5] >= tx0;
    const int xlo = s.v[2] < s.v[4] ? s.v[2] : s.v[4], xhi = s.v[2] < s.v[4] ? s.v[4] : s.v[2];
    const int ylo = s.v[3] < s.v[5] ? s.v[3] : s.v[5], yhi = s.v[3] < s.v[5] ? s.v[5] : s.v[3];
    return xlo <= tx1 && xhi >= tx0 && ylo <= ty1 && yhi >= ty0;
}

// Bits 0 .. rows - 1 (1 <= rows <= SEG_ROWS): bit r set iff t0 <= r <= t1.
HH_HD uint32_t seg_run_bits(long long t0, long long t1, int rows)
{
    if (t0 < 0) t0 = 0;
    if (t1 > rows - 1) t1 = rows - 1;
    if (t0 > t1) return 0u;
    return (~0u >> (31 - (int)t1)) & (~0u << (int)t0);
}

// The rows Y0 .. Y0 + rows - 1 of image column X that the line (xa, ya) -> (xb, yb) draws, as bits 0 .. rows - 1.  Every product in
// int64 (|coordinates| <= 2^23, so below 2^51).  Along x each column holds one pixel; along y the rows of a column are one run, found
// by inverting the rule: floor_div(2 t sx + dy, 2 dy) == k  <=>  2 dy k - dy <= 2 t sx <= 2 dy k + dy - 1.
HH_HD uint32_t seg_line_bits(int xa, int ya, int xb, int yb, int X, int Y0, int rows)
{
    const long long dx = xb > xa ? (long long)xb - xa : (long long)xa - xb, dy = yb > ya ? (long long)yb - ya : (long long)ya - yb;
    if (dx == 0 && dy == 0) return X == xa ? seg_run_bits((long long)ya - Y0, (long long)ya - Y0, rows) : 0u;
    if (dx >= dy) {
        if (xa > xb) { int t = xa; xa = xb; xb = t; t = ya; ya = yb; yb = t; }
        if (X < xa || X > xb) return 0u;
        const long long y = ya + seg_floor_div(2 * ((long long)X - xa) * ((long long)yb - ya) + dx, 2 * dx);
        return seg_run_bits(y - Y0, y - Y0, rows);
    }
    if (ya > yb) { int t = xa; xa = xb; xb = t; t = ya; ya = yb; yb = t; }
    if (X < (xa < xb ? xa : xb) || X > (xa < xb ? xb : xa) || Y0 > yb || Y0 + rows - 1 < ya) return 0u;
    const long long sx = (long long)xb - xa, k = (long long)X - xa;
    const long long lo = 2 * dy * k - dy, hi = 2 * dy * k + dy - 1;
    long long t0, t1;  // the run of t = y - ya with x == X
    if (sx == 0) {
        t0 = 0, t1 = dy;  // k == 0 here
    } else if (sx > 0) {
        t0 = seg_ceil_div(lo, 2 * sx), t1 = seg_floor_div(hi, 2 * sx);
    } else {
        t0 = seg_ceil_div(-hi, -2 * sx), t1 = seg_floor_div(-lo, -2 * sx);
    }
    if (t0 < 0) t0 = 0;
    if (t1 > dy) t1 = dy;
    return seg_run_bits(t0 + ya - Y0, t1 + ya - Y0, rows);
}

// The same for any surviving shape: a fill's bits are the toggle predicate of crowd_mask_math.h over its own toggles.
HH_HD uint32_t seg_item_bits(const SegItem &s, const uint32_t *toggles, int h, int X, int Y0, int rows)
{
    if (s.kind == HH_SEG_FILL) {
        if (X < s.c || X > s.d) return 0u;
        return crowd_column_bits(toggles + s.a, (uint32_t)s.b, (uint32_t)X * (uint32_t)h + (uint32_t)Y0, rows) & (~0u >> (32 - rows));
    }
    return seg_line_bits(s.a, s.b, s.c, s.d, X, Y0, rows);
}

HH_HD SegItem seg_item(const SegShape &s) { return SegItem{s.v[0], s.v[1], s.v[2], s.v[3], s.v[4], s.v[5]}; }

// One pixel: src = r | g << 8 | b << 16 as read, own = SEG_COVERED | colour or 0 -> the three bytes as stored (flags bit 0: B,G,R).
HH_HD uint32_t seg_pixel(uint32_t src, uint32_t own, float w0, float w1, int flags)
{
    const uint32_t ov = (own & SEG_COVERED) ? own : src;
    const uint32_t c0 = render_blend((uint8_t)(src & 255), (uint8_t)(ov & 255), w0, w1);
    const uint32_t c1 = render_blend((uint8_t)(src >> 8 & 255), (uint8_t)(ov >> 8 & 255), w0, w1);
    const uint32_t c2 = render_blend((uint8_t)(src >> 16 & 255), (uint8_t)(ov >> 16 & 255), w0, w1);
    return (flags & 1) ? (c2 | c1 << 8 | c0 << 16) : (c0 | c1 << 8 | c2 << 16);
}

// One frame on the host, in the kernel's own walk: tile by tile, the shapes culled chunk by chunk into a list in draw order, every
// (column, SEG_ROWS rows) cell of the tile walking the list with the last hit winning, then the blend row by row.  src may equal dst.
inline void seg_frame_host(const uint8_t *src, uint8_t *dst, const SegDesc &d, const SegShape *shapes, const uint32_t *toggles)
{
    const int h = d.h, w = d.w;
    std::vector<SegItem> list(SEG_CHUNK);
    std::vector<uint32_t> own((size_t)SEG_TH * SEG_TW);
    for (int ty0 = 0; ty0 < h; ty0 += SEG_TH)
        for (int tx0 = 0; tx0 < w; tx0 += SEG_TW) {
            const int ty1 = (ty0 + SEG_TH < h ? ty0 + SEG_TH : h) - 1, tx1 = (tx0 + SEG_TW < w ? tx0 + SEG_TW : w) - 1;
            std::fill(own.begin(), own.end(), 0u);
            draw_chunks_host(
                shapes + d.prim_offset, d.prim_count, SEG_CHUNK, list.data(), [&](const SegShape &s) { return seg_meets(s, tx0, ty0, tx1, ty1); }, seg_item,
                [&](int n) {
                    for (int t = 0; t < SEG_THREADS; ++t) {
                        const int col = t % SEG_TW, X = tx0 + col, Y0 = ty0 + t / SEG_TW * SEG_ROWS;
                        const int rows = (ty1 - Y0 + 1 < SEG_ROWS) ? ty1 - Y0 + 1 : SEG_ROWS;
                        if (X > tx1 || rows < 1) continue;
                        for (int k = 0; k < n; ++k) {
                            const uint32_t bits = seg_item_bits(list[k], toggles, h, X, Y0, rows);
                            for (int r = 0; r < rows; ++r)
                                if (bits >> r & 1) own[(size_t)(Y0 - ty0 + r) * SEG_TW + col] = SEG_COVERED | (uint32_t)list[k].colour;
                        }
                    }
                });
            for (int y = ty0; y <= ty1; ++y)
                for (int x = tx0; x <= tx1; ++x) {
                    const size_t at = ((size_t)y * w + x) * 3;
                    const uint32_t px = seg_pixel(src[at] | src[at + 1] << 8 | src[at + 2] << 16, own[(size_t)(y - ty0) * SEG_TW + x - tx0], d.w0, d.w1, d.flags);
                    dst[at] = px & 255, dst[at + 1] = px >> 8 & 255, dst[at + 2] = px >> 16 & 255;
                }
        }
}

// What hh_seg_overlay_u8_batch refuses for one frame, on the caller's host copies; nullptr = accepted.
inline const char *seg_check_frame(const SegDesc &d, const SegShape *shapes, long long num_shapes, const uint32_t *toggles, long long num_toggles)
{
    const long long bytes = (long long)d.h * d.w * 3;  // (reported only once the size and the offsets' sign have passed)
    const bool overlap = d.dst_offset != d.src_offset && d.dst_offset < d.src_offset + bytes && d.src_offset < d.dst_offset + bytes;
    if (const char *why = draw_check_frame(d, overlap ? "dst partially overlaps src" : nullptr, num_shapes, HH_SEG_MAX_SHAPES, "shape range outside the table",
                                           "more than HH_SEG_MAX_SHAPES shapes in one frame", "blend weight not finite or above 1e6 in magnitude"))
        return why;
    if (d.flags & ~1) return "unknown flag";
    if (d.reserved) return "non-zero reserved field";
    const uint32_t area = (uint32_t)d.h * (uint32_t)d.w;
    for (int i = 0; i < d.prim_count; ++i) {
        const int32_t *v = shapes[d.prim_offset + i].v;
        if (v[0] != HH_SEG_FILL && v[0] != HH_SEG_LINE) return "unknown shape kind";
        if (v[1] < 0 || v[1] > 0xFFFFFF) return "colour above 0xFFFFFF";
        if (v[6] || v[7]) return "non-zero reserved ints";
        if (v[0] == HH_SEG_LINE) {
            for (int j = 2; j < 6; ++j)
                if (v[j] < -SEG_MAX_COORD || v[j] > SEG_MAX_COORD) return "line endpoint beyond 2^23";
            continue;
        }
        if (v[2] < 0 || v[3] < 0 || (long long)v[2] + v[3] > num_toggles) return "toggle range outside the table";
        if (v[4] < 0 || v[5] >= d.w || v[4] > v[5]) return "column range outside the image";
        const uint32_t *t = toggles + v[2];
        for (int j = 0; j < v[3]; ++j) {
            if (t[j] > area) return "toggle above h*w";
            if (j && t[j] <= t[j - 1]) return "toggles not strictly increasing";
        }
        if (v[3] > 0 && t[0] < area) {  // as crowd_check_mask: the range must hold every covered column, else the cull would change the result
            const int first = (int)(t[0] / (uint32_t)d.h), last = (v[3] & 1) ? d.w - 1 : (int)((t[v[3] - 1] - 1) / (uint32_t)d.h);
            if (v[4] > first || v[5] < last) return "column range does not hold the fill";
        }
    }
    return nullptr;
}
#endif
