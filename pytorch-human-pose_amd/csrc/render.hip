// Pose overlays on the GPU: keypoints/visualization.py:13-90 (plot_connections with draw_elipsis) for a batch of frames of mixed sizes
// in ONE launch, and the general 8-bit cv2.resize(src, (W, H)) that the video path applies to the finished frame.  The drawing rule
// (which pixels a disc, a ring and a limb ellipse cover, the blend) is stated at hh_render_poses_u8_batch in include/hhrnet.h; its
// arithmetic is render_math.h, shared with the host.  The host forms the primitive table (hh_render_prim, draw order) and one
// hh_render_desc per frame; nothing but per-pixel work happens here.
//
// render_poses_kernel: a workgroup of 256 threads owns one RENDER_TH x RENDER_TW = 16 x 64 tile of one frame's output, a thread
// RENDER_PX = 4 horizontally adjacent pixels of it (draw_dev.h: draw_tile).  The frame's primitives are walked RENDER_CHUNK = 256 at
// a time: each lane tests one primitive's box against the tile, the survivors are compacted into LDS in draw order (draw_dev.h:
// draw_cull_slot), and every thread walks that list with render_inside, a later hit overwriting an earlier one.  Chunks
// follow each other in draw order and a thread keeps its pixels' current colours in registers across them, so the order holds across
// chunks and the list never needs more than one chunk of room (8 KB), whatever the frame's primitive count.  All lanes read the same
// list entry at the same time: an LDS broadcast, no bank conflict.  Then the thread blends against the source pixels it read once at
// the start and stores: every output byte is written exactly once by exactly one thread, no atomics, no global scratch.  A frame
// without primitives is blended and written all the same.  Loads and stores are dwords where the 12 bytes of a thread's four pixels
// are 4-byte aligned (frames whose row bytes are a multiple of 4, at an aligned offset), bytes otherwise and at the right edge.
//
// resize_u8_kernel: the streaming kernel of train_mosaic.hip without its restrictions: any h, w, H, W >= 1, 1 or 3 channels, the same
// taps (resize_dev.h) and the 2 x 2 mean at an exact factor of 2 on both axes.
#include "kernels.h"
#include "draw_dev.h"
#include "render_math.h"
#include "resize_dev.h"

#define RENDER_WAVES (RENDER_THREADS / 64)

__global__ __launch_bounds__(RENDER_THREADS) void render_poses_kernel(unsigned char *base, const RenderDesc *__restrict__ descs,
                                                                      const RenderPrim *__restrict__ prims)
{
    __shared__ RenderPrim list[RENDER_CHUNK];
    __shared__ int wave_count[RENDER_WAVES];
    const RenderDesc d = descs[blockIdx.z];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const DrawTile t = draw_tile(blockIdx.x, (d.w + RENDER_TW - 1) / RENDER_TW, d.h, d.w, tid);
    if (t.ty0 >= d.h) return;  // (the whole workgroup: the grid is sized for the largest frame of the batch)
    const int tx0 = t.tx0, ty0 = t.ty0, tx1 = t.tx1, ty1 = t.ty1, y = t.y, x = t.x, npx = t.npx;

    // the source pixels, read once: y < h and x + e < w for e < npx, so every byte is inside the frame's h * w * 3
    uint8_t sp[RENDER_PX * 3];
    const size_t at = ((size_t)(npx > 0 ? y : 0) * d.w + (npx > 0 ? x : 0)) * 3;
#pragma unroll
    for (int i = 0; i < RENDER_PX * 3; ++i) sp[i] = 0;
    const unsigned char *sptr = base + d.src_offset + at;
    if (npx == RENDER_PX && ((uintptr_t)sptr & 3) == 0) {
        draw_load_dwords<3>(sptr, [&](int i, uint32_t v) { sp[i] = v; });
    } else {
#pragma unroll
        for (int e = 0; e < RENDER_PX; ++e)
            if (e < npx) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) sp[e * 3 + ch] = sptr[e * 3 + ch];
            }
    }
    uint32_t conn[RENDER_PX];  // connections_image = image.copy(): r | g << 8 | b << 16
#pragma unroll
    for (int e = 0; e < RENDER_PX; ++e) conn[e] = sp[e * 3] | sp[e * 3 + 1] << 8 | sp[e * 3 + 2] << 16;

    for (int chunk = 0; chunk < d.prim_count; chunk += RENDER_CHUNK) {  // (uniform over the workgroup)
        const int i = chunk + tid;
        RenderPrim mine;
        bool keep = false;
        if (i < d.prim_count) {  // prim_offset + i < the table's length: checked on the host
            mine = prims[d.prim_offset + i];
            keep = render_box_meets(mine, tx0, ty0, tx1, ty1);
        }
        const DrawSlot cull = draw_cull_slot<RENDER_WAVES>(keep, lane, wave, wave_count);
        if (keep) list[cull.slot] = mine;  // < cull.total <= RENDER_CHUNK
        __syncthreads();
        if (npx > 0)
            for (int k = 0; k < cull.total; ++k) {
                const RenderPrim p = list[k];
                if (y < p.y0 || y > p.y1 || x + RENDER_PX - 1 < p.x0 || x > p.x1) continue;
                const uint32_t colour = p.rgb[0] | p.rgb[1] << 8 | p.rgb[2] << 16;
#pragma unroll
                for (int e = 0; e < RENDER_PX; ++e)
                    if (render_inside(p, x + e, y)) conn[e] = colour;
            }
        __syncthreads();  // the next chunk overwrites the list and the counts
    }
    if (npx <= 0) return;

    const bool bgr = d.flags & 1;
    uint8_t op[RENDER_PX * 3];
#pragma unroll
    for (int e = 0; e < RENDER_PX; ++e)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            op[e * 3 + (bgr ? 2 - ch : ch)] = render_blend(sp[e * 3 + ch], (conn[e] >> (8 * ch)) & 255, d.w0, d.w1);
    unsigned char *optr = base + d.dst_offset + at;
    if (npx == RENDER_PX && ((uintptr_t)optr & 3) == 0) {
        draw_store_dwords<3>(optr, [&](int i) { return op[i]; });
    } else {
#pragma unroll
        for (int e = 0; e < RENDER_PX; ++e)
            if (e < npx) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) optr[e * 3 + ch] = op[e * 3 + ch];
            }
    }
}

hipError_t launch_render_poses(unsigned char *base, const RenderDesc *descs, const RenderPrim *prims, int n, int max_tiles, hipStream_t s)
{
    hipLaunchKernelGGL(render_poses_kernel, dim3(max_tiles, 1, n), dim3(RENDER_THREADS), 0, s, base, descs, prims);
    return hipGetLastError();
}

void render_debug_host(const unsigned char *src, unsigned char *dst, const RenderDesc &d, const RenderPrim *prims)
{
    RenderPrim list[RENDER_CHUNK];
    render_frame_host(src, dst, d, prims, list);
}

#define RESIZE_PX 4     // output pixels per thread and row
#define RESIZE_TX 64    // threads along x: a block spans 256 output columns
#define RESIZE_TY 4     // thread rows
#define RESIZE_ROWS 4   // output rows per thread (rows yi, yi + RESIZE_TY, ...): a block spans 16 output rows

template <int CH>
__global__ __launch_bounds__(RESIZE_TX *RESIZE_TY) void resize_u8_kernel(const unsigned char *__restrict__ src, int h, int w, unsigned char *__restrict__ dst,
                                                                         int H, int W, int xtiles, double scale_x, double scale_y)
{
    const int xi = threadIdx.x % RESIZE_TX, yi = threadIdx.x / RESIZE_TX;
    const int x0 = ((int)(blockIdx.x % xtiles) * RESIZE_TX + xi) * RESIZE_PX;
    const int ybase = (int)(blockIdx.x / xtiles) * (RESIZE_TY * RESIZE_ROWS) + yi;
    if (x0 >= W) return;
    const int npx = min(RESIZE_PX, W - x0);
    const bool area = h == 2 * H && w == 2 * W;  // both scales exactly 2: OpenCV takes INTER_AREA's 2 x 2 mean

    AxisTap tx[RESIZE_PX];
#pragma unroll
    for (int e = 0; e < RESIZE_PX; ++e) tx[e] = axis_tap(min(x0 + e, W - 1), w, scale_x, true);  // (a clamped column is computed, never stored)

#pragma unroll 1
    for (int r = 0; r < RESIZE_ROWS; ++r) {
        const int y = ybase + r * RESIZE_TY;
        if (y >= H) break;
        unsigned char px[RESIZE_PX * CH];
        if (area) {
            // source rows 2y, 2y + 1 and columns 2x, 2x + 1 with x <= W - 1: all inside the 2H x 2W source; byte indices < h * w * CH < 2^31
#pragma unroll
            for (int e = 0; e < RESIZE_PX; ++e) {
                const int xs = 2 * min(x0 + e, W - 1);
                const unsigned char *p0 = src + ((2 * y) * w + xs) * CH, *p1 = p0 + w * CH;
#pragma unroll
                for (int c = 0; c < CH; ++c) px[e * CH + c] = (unsigned char)((p0[c] + p0[CH + c] + p1[c] + p1[CH + c] + 2) >> 2);
            }
        } else {
            const AxisTap ty = axis_tap(y, h, scale_y, false);
            // i0, i1 lie in [0, h - 1] resp. [0, w - 1] by construction: every byte index is < h * w * CH < 2^31 (checked by the caller)
            const unsigned char *p0 = src + ty.i0 * w * CH, *p1 = src + ty.i1 * w * CH;
#pragma unroll
            for (int e = 0; e < RESIZE_PX; ++e) {
                const int a = tx[e].i0, b = tx[e].i1, wa = tx[e].w0, wb = tx[e].w1;
#pragma unroll
                for (int c = 0; c < CH; ++c)
                    px[e * CH + c] = (unsigned char)vertical_pass(p0[a * CH + c] * wa + p0[b * CH + c] * wb, p1[a * CH + c] * wa + p1[b * CH + c] * wb, ty.w0, ty.w1);
            }
        }
        unsigned char *o = dst + ((size_t)y * W + x0) * CH;  // y < H, x0 + e < W for e < npx
        if (npx == RESIZE_PX && ((uintptr_t)o & 3) == 0) {
            draw_store_dwords<CH>(o, [&](int i) { return px[i]; });
        } else {
#pragma unroll
            for (int i = 0; i < RESIZE_PX * CH; ++i)
                if (i < npx * CH) o[i] = px[i];
        }
    }
}

// scale_x, scale_y: the source step per destination pixel, formed in double by the caller (cv2.resize's scale_x = 1 / inv_scale_x)
static hipError_t resize_u8(const unsigned char *src, int h, int w, int channels, unsigned char *dst, int H, int W, double scale_x, double scale_y, hipStream_t s)
{
    const int xtiles = (W + RESIZE_TX * RESIZE_PX - 1) / (RESIZE_TX * RESIZE_PX), ytiles = (H + RESIZE_TY * RESIZE_ROWS - 1) / (RESIZE_TY * RESIZE_ROWS);
    const dim3 grid(xtiles * ytiles), block(RESIZE_TX * RESIZE_TY);
    if (channels == 3) hipLaunchKernelGGL(resize_u8_kernel<3>, grid, block, 0, s, src, h, w, dst, H, W, xtiles, scale_x, scale_y);
    else hipLaunchKernelGGL(resize_u8_kernel<1>, grid, block, 0, s, src, h, w, dst, H, W, xtiles, scale_x, scale_y);
    return hipGetLastError();
}

// cv2.resize(src, (W, H)): inv_scale = (double)W / w, scale = 1 / inv_scale
hipError_t launch_resize_u8(const unsigned char *src, int h, int w, int channels, unsigned char *dst, int H, int W, hipStream_t s)
{
    return resize_u8(src, h, w, channels, dst, H, W, 1.0 / ((double)W / (double)w), 1.0 / ((double)H / (double)h), s);
}

// cv2.resize(src, (0, 0), fx=fx, fy=fy): the destination size H x W = cvRound(h fy) x cvRound(w fx) is formed by the caller; scale = 1 / f
hipError_t launch_resize_u8_scaled(const unsigned char *src, int h, int w, int channels, unsigned char *dst, int H, int W, double fx, double fy, hipStream_t s)
{
    return resize_u8(src, h, w, channels, dst, H, W, 1.0 / fx, 1.0 / fy, s);
}
