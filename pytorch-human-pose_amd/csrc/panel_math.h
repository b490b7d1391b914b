// The arithmetic of the heatmap panels (panels.hip; the per-pixel rule is stated at hh_heatmap_panels_u8 in include/hhrnet.h), kept apart
// from the kernels so that the same text also compiles for the host (hh_debug_heatmap_panels_host, tools/panels_host_check.cpp): the map
// descriptor, the value of a map at a pixel for the four source kinds, clip / min-max / quantise / colour / blend, the un-normalise, a
// whole figure in plain loops, and the validation.  Compile with -ffp-contract=off: every fp32 operation below rounds on its own; the
// only fused multiply-adds are the explicit ones of the bilinear (decode_dev.h has the same ones, and fmaf on the host is exact).
//
// Under hipcc the device side of panel_value() calls src_index() / bilerp() of decode_dev.h as they are; the host side calls the two
// __host__ overloads below, the same expressions (tests/test_panels_cpu.py and tests/test_gpu_panels.py hold both to tests/panels_ref.py
// byte for byte).  A plain C++ compiler sees only the host pair.
#ifndef HH_PANEL_MATH_H
#define HH_PANEL_MATH_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/hhrnet.h"
#include "host_dev.h"
#if defined(__HIPCC__)
#include "decode_dev.h"  // Lin, src_index, bilerp (device)
#else
struct Lin { int i0, i1; float w0, w1; };
#endif

// The launch geometry.  Paint: the drawing tile of host_dev.h on the canvas; the cells are culled against it one per lane, so a figure
// has at most HH_PANEL_MAX_MAPS = the workgroup's size maps.  Min/max: HH_PANEL_PARTS workgroups per map, each leaving one (max, min).
enum { PANEL_TH = DRAW_TH, PANEL_TW = DRAW_TW, PANEL_PX = DRAW_PX, PANEL_THREADS = DRAW_THREADS };
static_assert(PANEL_THREADS == HH_PANEL_MAX_MAPS, "one lane per map of a figure");

using PanelMap = hh_panel_map;
static_assert(sizeof(hh_panel_map) == 40, "ABI 3");

// F.interpolate(mode="bilinear", align_corners=False) of torch CPU: the host forms of decode_dev.h's src_index / bilerp (unqualified = host).
inline Lin src_index(int in_size, float scale, int dst)
{
    float r = fmaf(scale, (float)dst + 0.5f, -0.5f);
    if (r < 0.f) r = 0.f;
    const int a = (int)r;
    float l1 = r - (float)a;
    l1 = fminf(fmaxf(l1, 0.f), 1.f);
    Lin o;
    o.i0 = a; o.i1 = a + (a < in_size - 1 ? 1 : 0); o.w1 = l1; o.w0 = 1.f - l1;
    return o;
}
inline float bilerp(const float *img, int w, const Lin &ly, const Lin &lx)
{
    const float *r0 = img + (size_t)ly.i0 * w, *r1 = img + (size_t)ly.i1 * w;
    const float a = fmaf(r0[lx.i0], lx.w0, r0[lx.i1] * lx.w1);
    const float b = fmaf(r1[lx.i0], lx.w0, r1[lx.i1] * lx.w1);
    return fmaf(a, ly.w0, b * ly.w1);
}

HH_HD float panel_fma(float a, float b, float c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_fmaf(a, b, c);
#else
    return fmaf(a, b, c);
#endif
}

// One half-resolution tap (r, c) of a NESTED / AVERAGE map: the quarter-resolution map resized x2 (avg_at of decode_dev.h), for AVERAGE
// then averaged with the half-resolution stage.  Every index read lies inside [0, h) x [0, w) resp. [0, 2h) x [0, 2w) by src_index.
HH_HD float panel_half_tap(const PanelMap &m, int r, int c)
{
    const float up = bilerp(m.src, m.w, src_index(m.h, 0.5f, r), src_index(m.w, 0.5f, c));
    if (m.kind == HH_PANEL_NESTED) return up;
    return (up + m.src2[(size_t)r * (2 * m.w) + c]) / 2.0f;
}

// The value of map m at pixel (y, x) of its H x W cell, 0 <= y < H, 0 <= x < W.
HH_HD float panel_value(const PanelMap &m, int H, int W, int y, int x)
{
    if (m.kind == HH_PANEL_DIRECT) return m.src[(size_t)y * W + x];
    if (m.kind == HH_PANEL_SINGLE) {
        const float sy = (float)m.h / (float)H, sx = (float)m.w / (float)W;  // torch's area_pixel_compute_scale, as hh_decode forms it
        return bilerp(m.src, m.w, src_index(m.h, sy, y), src_index(m.w, sx, x));
    }
    // NESTED / AVERAGE: H == 4h, W == 4w; heat_at's default path of decode_dev.h
    const int hh = 2 * m.h, wh = 2 * m.w;
    const float sy = (float)hh / (float)H, sx = (float)wh / (float)W;
    const Lin ly = src_index(hh, sy, y), lx = src_index(wh, sx, x);
    const float a = panel_fma(panel_half_tap(m, ly.i0, lx.i0), lx.w0, panel_half_tap(m, ly.i0, lx.i1) * lx.w1);
    const float c = panel_fma(panel_half_tap(m, ly.i1, lx.i0), lx.w0, panel_half_tap(m, ly.i1, lx.i1) * lx.w1);
    return panel_fma(a, ly.w0, c * ly.w1);
}

// Step 1: np.clip(v, 0, 1); NaN stays NaN.
HH_HD float panel_clip(float v, int flags)
{
    if (flags & HH_PANEL_CLIP) v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
    return v;
}

// The running (max, min) of a map in np.max / np.min semantics: a NaN makes both NaN.  (fmaxf / fminf would drop it.)
struct PanelRange { float mx, mn; };
HH_HD PanelRange panel_range_first(float v) { PanelRange r; r.mx = v; r.mn = v; return r; }
HH_HD PanelRange panel_range_join(PanelRange a, PanelRange b)
{
    PanelRange r;
    if (a.mx != a.mx || b.mx != b.mx) { r.mx = r.mn = NAN; return r; }
    r.mx = a.mx > b.mx ? a.mx : b.mx;
    r.mn = a.mn < b.mn ? a.mn : b.mn;
    return r;
}

// Step 3: (uint8)(q) as numpy casts it: truncated toward zero as int32 (0 when q is not finite or outside int32), low 8 bits.
HH_HD int panel_level(float q)
{
    int t = 0;
    if (q >= -2147483648.f && q < 2147483648.f) t = (int)q;
    return t & 255;
}
HH_HD int panel_level_f64(double q)
{
    int t = 0;
    if (q >= -2147483648.0 && q < 2147483648.0) t = (int)q;
    return t & 255;
}

// addWeighted(img, 0.25, colour, 0.75, 0) on one channel: render_blend of render_math.h with fixed weights.
HH_HD uint8_t panel_blend(uint8_t img, uint8_t colour)
{
    const float a = (float)img * 0.25f, b = (float)colour * 0.75f;
    float v = rintf(a + b);
    v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
    return (uint8_t)(int)v;
}

// Steps 2-4: the value after step 1 -> index into the colour table.
HH_HD int panel_colour_index(float v, int flags, PanelRange r)
{
    if (flags & HH_PANEL_MINMAX) v = (v - r.mx) / (r.mx - r.mn);
    return 255 - panel_level(v * 255.0f);
}

// KeypointsTransform.inverse_transform on one element: ((double)x * std + mean) * 255 in float64, then the cast of step 3.
HH_HD uint8_t panel_unnormalize(float x, double sd, double mean)
{
    const double p = (double)x * sd;
    const double s = p + mean;
    return (uint8_t)panel_level_f64(s * 255.0);
}

// What hh_heatmap_panels_u8 refuses, on the caller's host copy of the table; nullptr = accepted.
inline const char *panel_check(const PanelMap *maps, int n, int H, int W, int Hc, int Wc, long long pitch)
{
    if (n < 1 || n > HH_PANEL_MAX_MAPS) return "need 1..HH_PANEL_MAX_MAPS (256) maps";
    if (H < 1 || W < 1 || Hc < 1 || Wc < 1 || H > 16384 || W > 16384 || Hc > 16384 || Wc > 16384) return "cell or canvas side outside 1..16384";
    if (pitch < (long long)Wc * 3) return "pitch smaller than a canvas row";
    if (pitch > (1ll << 30)) return "pitch beyond 2^30 bytes";
    for (int i = 0; i < n; ++i) {
        const PanelMap &m = maps[i];
        if (m.kind < HH_PANEL_DIRECT || m.kind > HH_PANEL_AVERAGE) return "unknown map kind";
        if (m.flags & ~(HH_PANEL_CLIP | HH_PANEL_MINMAX)) return "unknown flag";
        if (!m.src || (m.kind == HH_PANEL_AVERAGE && !m.src2)) return "null map pointer";
        if (m.h < 1 || m.w < 1 || m.h > 16384 || m.w > 16384) return "source side outside 1..16384";
        if (m.kind == HH_PANEL_DIRECT && (m.h != H || m.w != W)) return "a DIRECT map must have the cell's size";
        if ((m.kind == HH_PANEL_NESTED || m.kind == HH_PANEL_AVERAGE) && (4 * m.h != H || 4 * m.w != W)) return "a NESTED or AVERAGE map must be a quarter of the cell's size";
        if (m.oy < 0 || m.ox < 0 || (long long)m.oy + H > Hc || (long long)m.ox + W > Wc) return "cell outside the canvas";
    }
    return nullptr;
}

// One figure on the host: every map's range where it is asked for, the canvas zeroed, then the cells in table order (of two cells that
// overlap the later one wins, as on the device).  `ranges` is the caller's scratch of n entries.
inline void panel_figure_host(const PanelMap *maps, int n, const uint8_t *image, int H, int W, const uint8_t *lut, uint8_t *canvas, int Hc, int Wc,
                              long long pitch, PanelRange *ranges)
{
    for (int i = 0; i < n; ++i) {
        ranges[i] = panel_range_first(0.f);
        if (!(maps[i].flags & HH_PANEL_MINMAX)) continue;
        PanelRange r = panel_range_first(panel_clip(panel_value(maps[i], H, W, 0, 0), maps[i].flags));
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) r = panel_range_join(r, panel_range_first(panel_clip(panel_value(maps[i], H, W, y, x), maps[i].flags)));
        ranges[i] = r;
    }
    for (int y = 0; y < Hc; ++y)
        for (int b = 0; b < Wc * 3; ++b) canvas[(size_t)y * pitch + b] = 0;
    for (int i = 0; i < n; ++i) {
        const PanelMap &m = maps[i];
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const int c = panel_colour_index(panel_clip(panel_value(m, H, W, y, x), m.flags), m.flags, ranges[i]);
                uint8_t *o = canvas + (size_t)(m.oy + y) * pitch + (size_t)(m.ox + x) * 3;
                for (int ch = 0; ch < 3; ++ch) o[ch] = panel_blend(image[((size_t)y * W + x) * 3 + ch], lut[c * 3 + ch]);
            }
    }
}
#endif
