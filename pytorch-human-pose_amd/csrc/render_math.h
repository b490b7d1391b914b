// The arithmetic of the pose overlay (render.hip; the drawing rule is stated at hh_render_poses_u8_batch in include/hhrnet.h), kept
// apart from the kernel so that the same text also compiles for the host (hh_debug_render_host, tools/render_host_check.cpp): the
// primitive and frame descriptors, the tile cull, the inside test of the three primitive kinds, the blend, and a whole frame walked
// tile by tile in plain loops.  Compile with -ffp-contract=off: every fp32 operation below rounds on its own.
#ifndef HH_RENDER_MATH_H
#define HH_RENDER_MATH_H
#include <math.h>
#include <stdint.h>

#include "../../include/hhrnet.h"
#include "host_dev.h"

// The launch geometry, reported by hh_render_config: the drawing tile of host_dev.h on the output; the frame's primitives are culled
// against the tile RENDER_CHUNK at a time, one per lane.
enum { RENDER_TH = DRAW_TH, RENDER_TW = DRAW_TW, RENDER_PX = DRAW_PX, RENDER_THREADS = DRAW_THREADS, RENDER_CHUNK = DRAW_THREADS };

using RenderPrim = hh_render_prim;
using RenderDesc = hh_render_desc;
static_assert(sizeof(hh_render_prim) == 32 && sizeof(hh_render_desc) == 48, "ABI 3");

// Does the primitive's box meet the tile [tx0, tx1] x [ty0, ty1] (inclusive, already inside the frame)?
HH_HD bool render_box_meets(const RenderPrim &p, int tx0, int ty0, int tx1, int ty1)
{
    return p.x0 <= tx1 && p.x1 >= tx0 && p.y0 <= ty1 && p.y1 >= ty0;
}

// Is pixel (x, y) inside the primitive?  The box is a superset of every kind's set (the host forms it with a margin beyond the fp32
// rounding of the ellipse test), so testing it first changes nothing and keeps dx, dy small enough for the exact int32 forms:
// |dx|, |dy| <= 32767 inside a disc's or ring's box (render_check_frame), dx^2 + dy^2 < 2^31; an ellipse's dx, dy are exact in fp32.
HH_HD bool render_inside(const RenderPrim &p, int x, int y)
{
    if (x < p.x0 || x > p.x1 || y < p.y0 || y > p.y1) return false;
    const int dx = x - p.cx, dy = y - p.cy;
    if (p.kind == HH_RENDER_ELLIPSE) {
        // one order, every operation rounded to fp32: u = dx c + dy s, v = dy c - dx s, (2u B)^2 + (2v A)^2 <= (A B)^2
        const float fx = (float)dx, fy = (float)dy, Af = (float)p.A, Bf = (float)p.B;
        const float t0 = fx * p.c, t1 = fy * p.s, t2 = fy * p.c, t3 = fx * p.s;
        const float u = t0 + t1, v = t2 - t3;
        const float pu = (2.f * u) * Bf, qv = (2.f * v) * Af;
        const float pp = pu * pu, qq = qv * qv;
        const float lhs = pp + qq;
        const float ab = Af * Bf;
        const float rhs = ab * ab;
        return lhs <= rhs;
    }
    const int d2 = dx * dx + dy * dy, R = (int)p.A;
    if (p.kind == HH_RENDER_DISC) return d2 <= R * R + R;
    return d2 > R * R - R && d2 <= R * R + R;  // HH_RENDER_RING
}

// addWeighted on one channel: rintf(img w0 + conn w1), products and sum rounded separately, clamped to 0..255.
HH_HD uint8_t render_blend(uint8_t img, uint8_t conn, float w0, float w1)
{
    const float a = (float)img * w0, b = (float)conn * w1;
    float v = rintf(a + b);
    v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
    return (uint8_t)(int)v;
}

// The kernels' chunked cull on the host (the twins of render, text and seg): `count` items `chunk` at a time; of each chunk those
// that meets() accepts go through make() into `list` in draw order, and walk(n) applies the n listed ones.
template <class Src, class Item, class Meets, class Make, class Walk>
inline void draw_chunks_host(const Src *items, int count, int chunk, Item *list, Meets meets, Make make, Walk walk)
{
    for (int first = 0; first < count; first += chunk) {
        int n = 0;
        for (int i = first; i < count && i < first + chunk; ++i)
            if (meets(items[i])) list[n++] = make(items[i]);
        walk(n);
    }
}

// What every drawing call refuses in a frame's descriptor, in this order; nullptr = accepted.  `own`: the feature's refusal about the
// two offsets, if any; the other wordings are the feature's too; weight_why = nullptr: no blend weights in the descriptor.
inline const char *draw_check_frame(const hh_render_desc &d, const char *own, long long table_len, int max_prims, const char *range_why,
                                    const char *max_why, const char *weight_why)
{
    if (d.h < 1 || d.w < 1 || d.h > 16384 || d.w > 16384) return "frame size outside 1..16384";
    if (d.src_offset < 0 || d.dst_offset < 0) return "negative offset";
    if (own) return own;
    if (d.prim_count < 0 || d.prim_offset < 0 || (long long)d.prim_offset + d.prim_count > table_len) return range_why;
    if (d.prim_count > max_prims) return max_why;
    if (weight_why && (!(d.w0 == d.w0) || !(d.w1 == d.w1) || fabsf(d.w0) > 1e6f || fabsf(d.w1) > 1e6f)) return weight_why;
    return nullptr;
}

// One frame on the host, in the kernel's own walk: tile by tile, the primitives culled chunk by chunk into a list in draw order, every
// pixel walking the list with the last hit winning, then blended.  `list` is the caller's scratch of RENDER_CHUNK entries.
inline void render_frame_host(const uint8_t *src, uint8_t *dst, const RenderDesc &d, const RenderPrim *prims, RenderPrim *list)
{
    const int h = d.h, w = d.w;
    for (int ty0 = 0; ty0 < h; ty0 += RENDER_TH)
        for (int tx0 = 0; tx0 < w; tx0 += RENDER_TW) {
            const int ty1 = (ty0 + RENDER_TH < h ? ty0 + RENDER_TH : h) - 1, tx1 = (tx0 + RENDER_TW < w ? tx0 + RENDER_TW : w) - 1;
            uint8_t conn[RENDER_TH][RENDER_TW][3];
            for (int y = ty0; y <= ty1; ++y)
                for (int x = tx0; x <= tx1; ++x)
                    for (int ch = 0; ch < 3; ++ch) conn[y - ty0][x - tx0][ch] = src[((size_t)y * w + x) * 3 + ch];
            draw_chunks_host(
                prims + d.prim_offset, d.prim_count, RENDER_CHUNK, list, [&](const RenderPrim &p) { return render_box_meets(p, tx0, ty0, tx1, ty1); },
                [](const RenderPrim &p) { return p; },
                [&](int n) {
                    for (int y = ty0; y <= ty1; ++y)
                        for (int x = tx0; x <= tx1; ++x)
                            for (int i = 0; i < n; ++i)
                                if (render_inside(list[i], x, y)) {
                                    uint8_t *c = conn[y - ty0][x - tx0];
                                    c[0] = list[i].rgb[0], c[1] = list[i].rgb[1], c[2] = list[i].rgb[2];
                                }
                });
            for (int y = ty0; y <= ty1; ++y)
                for (int x = tx0; x <= tx1; ++x)
                    for (int ch = 0; ch < 3; ++ch) {
                        const size_t at = ((size_t)y * w + x) * 3;
                        dst[at + ((d.flags & 1) ? 2 - ch : ch)] = render_blend(src[at + ch], conn[y - ty0][x - tx0][ch], d.w0, d.w1);
                    }
        }
}

// What hh_render_poses_u8_batch refuses, on the caller's host copy; nullptr = accepted.  `max_prims` is HH_RENDER_MAX_PRIMS.
inline const char *render_check_frame(const RenderDesc &d, const RenderPrim *prims, long long table_len, int max_prims)
{
    if (const char *why = draw_check_frame(d, nullptr, table_len, max_prims, "primitive range outside the table",
                                           "more than HH_RENDER_MAX_PRIMS primitives in one frame", "blend weight not finite"))
        return why;
    if (d.flags & ~1) return "unknown flag";
    for (int i = 0; i < d.prim_count; ++i) {
        const RenderPrim &p = prims[d.prim_offset + i];
        if (p.kind > HH_RENDER_ELLIPSE) return "unknown primitive kind";
        if (p.A < 1 || p.B < 1) return "primitive with A or B < 1";
        if (p.kind != HH_RENDER_ELLIPSE && p.A > 32767) return "disc or ring radius above 32767";
        if (p.cx < -(1 << 23) || p.cx > (1 << 23) || p.cy < -(1 << 23) || p.cy > (1 << 23)) return "primitive centre beyond 2^23";
        if (p.x0 < 0 || p.y0 < 0 || p.x1 > 16383 || p.y1 > 16383) return "bounding box outside 0..16383";
        // the box may not reach further from the centre than the exact forms allow (an empty box is always fine)
        const long long reach = p.kind == HH_RENDER_ELLIPSE ? 65536 : 32767;
        if (p.x0 <= p.x1 && p.y0 <= p.y1 &&
            ((long long)p.x0 - p.cx < -reach || (long long)p.x1 - p.cx > reach || (long long)p.y0 - p.cy < -reach || (long long)p.y1 - p.cy > reach))
            return "bounding box too far from the centre (32767 for discs and rings, 65536 for ellipses)";
    }
    return nullptr;
}
#endif
