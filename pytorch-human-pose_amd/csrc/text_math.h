// The arithmetic of the text labels (text.hip; the rule is stated at hh_text_labels_u8_batch in include/hhrnet.h), kept apart from the
// kernel so that the same text also compiles for the host (hh_debug_text_host, tools/text_host_check.cpp): the two primitive kinds
// applied to one pixel, the list of tiles that a frame's primitives touch, one frame walked tile by tile in plain loops, and the
// validation.  Rows and descriptors are hh_render_prim and hh_render_desc, read as hh_text_labels_u8_batch states.
// Compile with -ffp-contract=off: every fp32 operation of the box blend rounds on its own.
#ifndef HH_TEXT_MATH_H
#define HH_TEXT_MATH_H
#include "render_math.h"

// The launch geometry, reported by hh_text_config: a workgroup of TEXT_THREADS owns one TEXT_TH x TEXT_TW tile of one frame, a thread
// TEXT_PX horizontally adjacent pixels of it; the frame's primitives are culled against the tile TEXT_CHUNK at a time, one per lane.
enum { TEXT_TH = DRAW_TH, TEXT_TW = DRAW_TW, TEXT_PX = DRAW_PX, TEXT_THREADS = DRAW_THREADS, TEXT_CHUNK = DRAW_THREADS };

using TextPrim = hh_text_prim;
using TextDesc = hh_text_desc;
struct TextTile { int32_t frame, tile; };  // tile = ty * xtiles + tx with xtiles = ceil(w / TEXT_TW)

HH_HD int text_xtiles(int w) { return (w + TEXT_TW - 1) / TEXT_TW; }
HH_HD int text_ytiles(int h) { return (h + TEXT_TH - 1) / TEXT_TH; }

// One primitive on one pixel that lies inside its box; `px` = r | g << 8 | b << 16 as stored.  A glyph's box lies inside its bitmap
// (text_check_frame), so the coverage index is inside [off, off + A * B), which lies inside the atlas.
HH_HD uint32_t text_apply(const TextPrim &p, const uint8_t *atlas, int x, int y, uint32_t px)
{
    if (p.kind == HH_TEXT_BOX) {
        if (p.A) return p.rgb[0] | p.rgb[1] << 8 | p.rgb[2] << 16;
        uint32_t out = 0;
        for (int ch = 0; ch < 3; ++ch) out |= (uint32_t)render_blend((px >> (8 * ch)) & 255, p.rgb[ch], p.c, p.s) << (8 * ch);
        return out;
    }
    const uint32_t c = atlas[(int)p.c + (y - p.cy) * (int)p.A + (x - p.cx)];
    uint32_t out = 0;
    for (int ch = 0; ch < 3; ++ch) out |= ((((px >> (8 * ch)) & 255) * (255u - c) + p.rgb[ch] * c + 127u) / 255u) << (8 * ch);
    return out;
}

// The tiles of frame `f` that some primitive's box touches, ascending; `seen` is the caller's scratch of ytiles * xtiles bytes.
// Counts all of them, stores the first `room`.
inline long long text_list_tiles(const TextDesc &d, const TextPrim *prims, int f, uint8_t *seen, TextTile *out, long long room)
{
    const int xt = text_xtiles(d.w), yt = text_ytiles(d.h);
    for (int i = 0; i < xt * yt; ++i) seen[i] = 0;
    for (int i = 0; i < d.prim_count; ++i) {
        const TextPrim &p = prims[d.prim_offset + i];
        if (p.x1 < p.x0 || p.y1 < p.y0) continue;
        for (int ty = p.y0 / TEXT_TH; ty <= p.y1 / TEXT_TH; ++ty)
            for (int tx = p.x0 / TEXT_TW; tx <= p.x1 / TEXT_TW; ++tx) seen[ty * xt + tx] = 1;
    }
    long long n = 0;
    for (int i = 0; i < xt * yt; ++i)
        if (seen[i]) {
            if (n < room) out[n] = TextTile{f, i};
            ++n;
        }
    return n;
}

// One tile of a frame on the host, in the kernel's own walk: the primitives culled chunk by chunk into a list in draw order, every
// pixel of the tile walking the list.  A pixel that no primitive covers is neither read nor written.  `list`: TEXT_CHUNK entries.
inline void text_tile_host(uint8_t *frame, const TextDesc &d, const TextPrim *prims, const uint8_t *atlas, int tile, TextPrim *list)
{
    const int xt = text_xtiles(d.w);
    const int ty0 = tile / xt * TEXT_TH, tx0 = tile % xt * TEXT_TW;
    const int ty1 = (ty0 + TEXT_TH < d.h ? ty0 + TEXT_TH : d.h) - 1, tx1 = (tx0 + TEXT_TW < d.w ? tx0 + TEXT_TW : d.w) - 1;
    draw_chunks_host(
        prims + d.prim_offset, d.prim_count, TEXT_CHUNK, list, [&](const TextPrim &p) { return render_box_meets(p, tx0, ty0, tx1, ty1); },
        [](const TextPrim &p) { return p; },
        [&](int n) {
            for (int i = 0; i < n; ++i) {
                const TextPrim &p = list[i];
                for (int y = p.y0 > ty0 ? p.y0 : ty0; y <= (p.y1 < ty1 ? p.y1 : ty1); ++y)
                    for (int x = p.x0 > tx0 ? p.x0 : tx0; x <= (p.x1 < tx1 ? p.x1 : tx1); ++x) {
                        uint8_t *q = frame + ((size_t)y * d.w + x) * 3;
                        const uint32_t v = text_apply(p, atlas, x, y, q[0] | q[1] << 8 | q[2] << 16);
                        q[0] = v & 255, q[1] = (v >> 8) & 255, q[2] = (v >> 16) & 255;
                    }
            }
        });
}

// What hh_text_labels_u8_batch refuses in one frame, on the caller's host copy; nullptr = accepted.
inline const char *text_check_frame(const TextDesc &d, const TextPrim *prims, long long table_len, long long atlas_len)
{
    const char *in_place = d.src_offset != d.dst_offset ? "frames are drawn in place: dst_offset must equal src_offset" : nullptr;
    if (const char *why = draw_check_frame(d, in_place, table_len, HH_TEXT_MAX_PRIMS, "primitive range outside the table",
                                           "more than HH_TEXT_MAX_PRIMS primitives in one frame", nullptr))
        return why;
    if (d.flags != 0 || d.reserved != 0) return "unknown flag";
    for (int i = 0; i < d.prim_count; ++i) {
        const TextPrim &p = prims[d.prim_offset + i];
        if (p.kind > HH_TEXT_GLYPH) return "unknown primitive kind";
        if (p.cx < -(1 << 23) || p.cx > (1 << 23) || p.cy < -(1 << 23) || p.cy > (1 << 23)) return "coordinate beyond 2^23";
        const bool empty = p.x1 < p.x0 || p.y1 < p.y0;
        if (!empty && (p.x0 < 0 || p.y0 < 0 || p.x1 >= d.w || p.y1 >= d.h)) return "box outside the frame";
        if (p.kind == HH_TEXT_BOX) {
            if (p.A > 1 || p.B != 0) return "unknown flag";
            if (!(fabsf(p.c) <= 1e6f) || !(fabsf(p.s) <= 1e6f)) return "blend weight not finite";
        } else {
            if (p.A < 1 || p.B < 1) return "empty or inverted glyph bitmap";
            if (!(p.c >= 0.f) || p.c >= 16777216.f || p.c != (float)(int)p.c || p.s != 0.f) return "glyph coverage offset is not an integer in 0..2^24 - 1";
            if ((long long)p.c + (long long)p.A * p.B > atlas_len) return "glyph coverage range leaves the atlas";
            if (!empty && (p.x0 < p.cx || p.y0 < p.cy || p.x1 > (long long)p.cx + p.A - 1 || p.y1 > (long long)p.cy + p.B - 1)) return "glyph box outside its bitmap";
        }
    }
    return nullptr;
}
#endif
