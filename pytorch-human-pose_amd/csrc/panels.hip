// Heatmap panels on the GPU: plot_heatmaps + make_grid of the reference (keypoints/visualization.py:93-110, utils/image.py:15-38) for all
// the grids of one figure in two launches, and KeypointsTransform.inverse_transform (base/transforms/base.py:33-41).  The per-pixel rule
// is stated at hh_heatmap_panels_u8 in include/hhrnet.h; its arithmetic is panel_math.h, shared with the host.  A full-resolution fp32
// map is never stored: both passes resample the stage outputs where they need a value (decode_dev.h's bilinear).
//
// panels_minmax_kernel: grid (HH_PANEL_PARTS, n).  The HH_PANEL_PARTS workgroups of a map that asks for min-max walk its H x W pixels
// interleaved, each thread keeping a running maximum, minimum and a saw-a-NaN bit; a wave reduces through shuffles, the four waves through
// LDS, and thread 0 stores the part's (max, min) pair, both NaN if any lane saw one.  Every pair that the paint pass reads is written
// by this launch, unconditionally: there is no atomic, no counter and nothing that has to be cleared between calls.  A part without
// pixels stores the identity (-inf, +inf).  Workgroups of maps without the flag return at once; the launch is skipped when no map has it.
//
// panels_paint_kernel: a workgroup of 256 threads owns one PANEL_TH x PANEL_TW = 16 x 64 tile of the canvas, a thread PANEL_PX = 4
// horizontally adjacent pixels of it (draw_dev.h: draw_tile).  Each lane tests one map's cell against the tile; the survivors are
// compacted into LDS in table order (the cull of draw_dev.h's draw_cull_slot, here with two arrays); each wave then joins the
// HH_PANEL_PARTS pairs of the listed maps that use min-max.  A pixel takes the last listed cell that holds it (a later map overwrites an earlier one) or is zero: padding and unused
// cells are written by the same launch.  Every canvas byte of the Wc * 3 row bytes is written exactly once by exactly one thread.  Cell
// origins and the pitch are arbitrary, so a thread's 12 bytes are stored as three dwords only when they are 4-byte aligned and all four
// pixels are inside the canvas, byte by byte otherwise (the right edge, and every row whose address is odd).
#include "kernels.h"
#include "draw_dev.h"
#include "panel_math.h"

#define PANEL_WAVES (PANEL_THREADS / 64)

__global__ __launch_bounds__(PANEL_THREADS) void panels_minmax_kernel(const PanelMap *__restrict__ maps, int H, int W, float *__restrict__ parts)
{
    __shared__ float smx[PANEL_WAVES], smn[PANEL_WAVES];
    __shared__ int sbad[PANEL_WAVES];
    const PanelMap m = maps[blockIdx.y];
    if (!(m.flags & HH_PANEL_MINMAX)) return;  // (the whole workgroup)
    const int total = H * W;                // <= 2^28 (checked by the caller)
    float mx = -INFINITY, mn = INFINITY;
    bool bad = false;
    for (int idx = (int)blockIdx.x * PANEL_THREADS + (int)threadIdx.x; idx < total; idx += HH_PANEL_PARTS * PANEL_THREADS) {
        const float v = panel_clip(panel_value(m, H, W, idx / W, idx % W), m.flags);
        bad |= v != v;
        mx = v > mx ? v : mx;
        mn = v < mn ? v : mn;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float omx = __shfl_xor(mx, off), omn = __shfl_xor(mn, off);
        mx = omx > mx ? omx : mx;
        mn = omn < mn ? omn : mn;
    }
    const int any_bad = __any(bad);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) smx[wave] = mx, smn[wave] = mn, sbad[wave] = any_bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        int b = 0;
#pragma unroll
        for (int v = 0; v < PANEL_WAVES; ++v) {
            mx = smx[v] > mx ? smx[v] : mx;
            mn = smn[v] < mn ? smn[v] : mn;
            b |= sbad[v];
        }
        float *o = parts + ((size_t)blockIdx.y * HH_PANEL_PARTS + blockIdx.x) * 2;  // < n * HH_PANEL_PARTS * 2 floats
        o[0] = b ? NAN : mx;
        o[1] = b ? NAN : mn;
    }
}

__global__ __launch_bounds__(PANEL_THREADS) void panels_paint_kernel(const PanelMap *__restrict__ maps, int n, const unsigned char *__restrict__ image, int H,
                                                                     int W, const unsigned char *__restrict__ lut, unsigned char *__restrict__ canvas, int Hc,
                                                                     int Wc, long long pitch, const float *__restrict__ parts, int xtiles)
{
    __shared__ PanelMap list[HH_PANEL_MAX_MAPS];
    __shared__ int list_index[HH_PANEL_MAX_MAPS];
    __shared__ PanelRange range[HH_PANEL_MAX_MAPS];
    __shared__ unsigned char slut[768];
    __shared__ int wave_count[PANEL_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const DrawTile t = draw_tile(blockIdx.x, xtiles, Hc, Wc, tid);  // inside the canvas by the grid's size
    const int tx0 = t.tx0, ty0 = t.ty0, tx1 = t.tx1, ty1 = t.ty1, y = t.y, x = t.x, npx = t.npx;
    for (int i = tid; i < 768; i += PANEL_THREADS) slut[i] = lut[i];

    PanelMap mine;
    bool keep = false;
    if (tid < n) {  // n <= HH_PANEL_MAX_MAPS = the workgroup's size
        mine = maps[tid];
        keep = mine.ox <= tx1 && mine.ox + W - 1 >= tx0 && mine.oy <= ty1 && mine.oy + H - 1 >= ty0;
    }
    // draw_dev.h's draw_cull_slot written out: through the helper this kernel's SGPR count goes from 33 to 37 (tools/isa_diff.py)
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wave_count[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int v = 0; v < PANEL_WAVES; ++v) {
        const int c = wave_count[v];
        before += v < wave ? c : 0;
        total += c;
    }
    if (keep) {
        const int at = before + __popcll(bal & ((1ull << lane) - 1ull));  // < total <= HH_PANEL_MAX_MAPS
        list[at] = mine;
        list_index[at] = tid;
    }
    __syncthreads();
    // the listed maps' ranges: wave v joins the parts of entries v, v + PANEL_WAVES, ... (uniform per wave)
    for (int k = wave; k < total; k += PANEL_WAVES) {
        PanelRange r = panel_range_first(0.f);
        if (list[k].flags & HH_PANEL_MINMAX) {
            const float *p = parts + (size_t)list_index[k] * HH_PANEL_PARTS * 2;
            r.mx = lane < HH_PANEL_PARTS ? p[lane * 2] : -INFINITY;
            r.mn = lane < HH_PANEL_PARTS ? p[lane * 2 + 1] : INFINITY;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                PanelRange o;
                o.mx = __shfl_xor(r.mx, off), o.mn = __shfl_xor(r.mn, off);
                r = panel_range_join(r, o);
            }
        }
        if (lane == 0) range[k] = r;
    }
    __syncthreads();

    if (npx <= 0) return;
    uint8_t op[PANEL_PX * 3];
#pragma unroll
    for (int e = 0; e < PANEL_PX; ++e) {
        op[e * 3] = op[e * 3 + 1] = op[e * 3 + 2] = 0;
        const int X = x + e;
        int hit = -1;
        for (int k = 0; k < total; ++k)
            if (y >= list[k].oy && y < list[k].oy + H && X >= list[k].ox && X < list[k].ox + W) hit = k;
        if (e < npx && hit >= 0) {
            const PanelMap m = list[hit];
            const int cy = y - m.oy, cx = X - m.ox;  // 0 <= cy < H, 0 <= cx < W
            const int c = panel_colour_index(panel_clip(panel_value(m, H, W, cy, cx), m.flags), m.flags, range[hit]);
            const unsigned char *ip = image + ((size_t)cy * W + cx) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) op[e * 3 + ch] = panel_blend(ip[ch], slut[c * 3 + ch]);
        }
    }
    unsigned char *optr = canvas + (size_t)y * pitch + (size_t)x * 3;  // y < Hc, x + e < Wc for e < npx: inside the row's Wc * 3 bytes
    if (npx == PANEL_PX && ((uintptr_t)optr & 3) == 0) {
        draw_store_dwords<3>(optr, [&](int i) { return op[i]; });
    } else {
#pragma unroll
        for (int i = 0; i < PANEL_PX * 3; ++i)
            if (i < npx * 3) optr[i] = op[i];
    }
}

hipError_t launch_panels(const PanelMap *maps, int n, bool any_minmax, const unsigned char *image, int H, int W, const unsigned char *lut,
                         unsigned char *canvas, int Hc, int Wc, long long pitch, float *parts, hipStream_t s)
{
    if (any_minmax) {
        hipLaunchKernelGGL(panels_minmax_kernel, dim3(HH_PANEL_PARTS, n), dim3(PANEL_THREADS), 0, s, maps, H, W, parts);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const int xtiles = (Wc + PANEL_TW - 1) / PANEL_TW, ytiles = (Hc + PANEL_TH - 1) / PANEL_TH;
    hipLaunchKernelGGL(panels_paint_kernel, dim3(xtiles * ytiles), dim3(PANEL_THREADS), 0, s, maps, n, image, H, W, lut, canvas, Hc, Wc, pitch, parts, xtiles);
    return hipGetLastError();
}

void panels_debug_host(const PanelMap *maps, int n, const unsigned char *image, int H, int W, const unsigned char *lut, unsigned char *canvas, int Hc,
                       int Wc, long long pitch, PanelRange *ranges)
{
    panel_figure_host(maps, n, image, H, W, lut, canvas, Hc, Wc, pitch, ranges);
}

// x fp32 [3,H,W] -> out uint8 [H,W,3]: a thread per pixel, the three planes read coalesced
__global__ __launch_bounds__(256) void unnormalize_u8_kernel(const float *__restrict__ x, int hw, unsigned char *__restrict__ out, double m0, double m1, double m2,
                                                             double s0, double s1, double s2)
{
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= hw) return;
    unsigned char *o = out + (size_t)i * 3;  // i < H * W: bytes 3i .. 3i + 2 of H * W * 3
    o[0] = panel_unnormalize(x[i], s0, m0);
    o[1] = panel_unnormalize(x[(size_t)hw + i], s1, m1);
    o[2] = panel_unnormalize(x[2 * (size_t)hw + i], s2, m2);
}

hipError_t launch_unnormalize_u8(const float *x, int H, int W, unsigned char *out, const double *mean, const double *stdv, hipStream_t s)
{
    const int hw = H * W;
    hipLaunchKernelGGL(unnormalize_u8_kernel, dim3((hw + 255) / 256), dim3(256), 0, s, x, hw, out, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2]);
    return hipGetLastError();
}
