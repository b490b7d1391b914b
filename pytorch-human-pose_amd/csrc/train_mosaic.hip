// The mosaic of the training input composed on the GPU: keypoints/datasets/coco.py:300-370 (get_raw_mosaiced_data) for all mosaic
// samples of a batch in ONE launch.  Four raw images and their crowd masks are resized to S x S each (cv2.resize(src, (S, S)),
// 8-bit INTER_LINEAR) and written into the quadrants of a uint8 RGB [2S,2S,3] canvas and a uint8 0 / 255 [2S,2S] mask canvas
// (hh_mosaic_desc of include/hhrnet.h).  The canvases are ordinary sources of hh_train_images_u8_batch / hh_train_masks_u8_batch.
//
// The resize is the one stated at hh_mosaic_u8_batch in include/hhrnet.h, all integer after the coordinates: per axis
// scale = 1.0 / ((double)S / src), f = (float)((d + 0.5) * scale - 0.5) with product and difference rounded separately (the file is
// compiled with -ffp-contract=off), two taps with 11-bit weights, the horizontal pass kept as int, the vertical pass with OpenCV's
// >> 4, >> 16, + 2, >> 2.  A source of exactly 2S x 2S takes the 2 x 2 mean (a + b + c + d + 2) >> 2 instead (OpenCV's INTER_AREA
// shortcut).  The mask canvas holds 255 where the resized 0 / 255 mask is non-zero.
//
// A streaming kernel: one thread produces MOSAIC_PX = 4 horizontally adjacent pixels of one tile row, image and mask, for
// MOSAIC_ROWS rows: 12 image bytes and 4 mask bytes per row, stored as three dwords and one (S % 4 == 0 and canvas offsets that are
// multiples of 4 make every store aligned; a wave stores 768 contiguous image bytes).  The column taps and weights of the four
// pixels are formed once per thread, the row taps and weights once per row.  The gathers are byte loads (at most 4 source pixels
// per output pixel); no LDS.  Every canvas byte is written exactly once by exactly one thread; nothing depends on the launch.
#include "kernels.h"
#include "draw_dev.h"
#include "resize_dev.h"

#define MOSAIC_PX 4     // output pixels per thread and row
#define MOSAIC_TX 64    // threads along x: a block spans 256 output columns
#define MOSAIC_TY 4     // thread rows
#define MOSAIC_ROWS 4   // output rows per thread (rows yi, yi + MOSAIC_TY, ...): a block spans 16 output rows

__global__ __launch_bounds__(MOSAIC_TX *MOSAIC_TY) void mosaic_kernel(unsigned char *base, const hh_mosaic_desc *__restrict__ descs, int S,
                                                                      int xtiles)
{
    const int xi = threadIdx.x % MOSAIC_TX, yi = threadIdx.x / MOSAIC_TX;
    const int quad = blockIdx.y;
    const hh_mosaic_desc &d = descs[blockIdx.z];
    const int h = d.tile[quad].h, w = d.tile[quad].w;
    const unsigned char *img = base + d.tile[quad].image_offset, *msk = base + d.tile[quad].mask_offset;
    const int x0 = ((int)(blockIdx.x % xtiles) * MOSAIC_TX + xi) * MOSAIC_PX;  // S % 4 == 0: a thread's four pixels are all inside or all outside
    const int ybase = (int)(blockIdx.x / xtiles) * (MOSAIC_TY * MOSAIC_ROWS) + yi;
    if (x0 >= S) return;

    const int C2 = 2 * S;  // canvas side
    unsigned char *cimg = base + d.canvas_image_offset + ((size_t)(quad >> 1) * S * C2 + (size_t)(quad & 1) * S + x0) * 3;
    unsigned char *cmsk = base + d.canvas_mask_offset + (size_t)(quad >> 1) * S * C2 + (size_t)(quad & 1) * S + x0;
    const bool area = h == C2 && w == C2;  // both scales exactly 2: OpenCV takes INTER_AREA's 2 x 2 mean
    const double scale_x = 1.0 / ((double)S / (double)w), scale_y = 1.0 / ((double)S / (double)h);

    AxisTap tx[MOSAIC_PX];
#pragma unroll
    for (int e = 0; e < MOSAIC_PX; ++e) tx[e] = axis_tap(x0 + e, w, scale_x, true);

#pragma unroll 1
    for (int r = 0; r < MOSAIC_ROWS; ++r) {
        const int y = ybase + r * MOSAIC_TY;
        if (y >= S) break;
        unsigned char px[MOSAIC_PX * 3], mk[MOSAIC_PX];
        if (area) {
            // source rows 2y, 2y + 1 and columns 2(x0 + e), 2(x0 + e) + 1: all inside the 2S x 2S source; byte indices < h * w * 3 < 2^31
            const unsigned char *p0 = img + ((2 * y) * w + 2 * x0) * 3, *p1 = p0 + w * 3;
            const unsigned char *m0 = msk + (2 * y) * w + 2 * x0, *m1 = m0 + w;
#pragma unroll
            for (int e = 0; e < MOSAIC_PX; ++e) {
#pragma unroll
                for (int c = 0; c < 3; ++c) px[e * 3 + c] = (unsigned char)((p0[e * 6 + c] + p0[e * 6 + 3 + c] + p1[e * 6 + c] + p1[e * 6 + 3 + c] + 2) >> 2);
                mk[e] = ((m0[e * 2] + m0[e * 2 + 1] + m1[e * 2] + m1[e * 2 + 1] + 2) >> 2) ? 255 : 0;
            }
        } else {
            const AxisTap ty = axis_tap(y, h, scale_y, false);
            // i0, i1 lie in [0, h - 1] resp. [0, w - 1] by construction: every byte index is < h * w * 3 < 2^31 (checked by the caller)
            const unsigned char *p0 = img + ty.i0 * w * 3, *p1 = img + ty.i1 * w * 3;
            const unsigned char *m0 = msk + ty.i0 * w, *m1 = msk + ty.i1 * w;
#pragma unroll
            for (int e = 0; e < MOSAIC_PX; ++e) {
                const int a = tx[e].i0, b = tx[e].i1, wa = tx[e].w0, wb = tx[e].w1;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    px[e * 3 + c] = (unsigned char)vertical_pass(p0[a * 3 + c] * wa + p0[b * 3 + c] * wb, p1[a * 3 + c] * wa + p1[b * 3 + c] * wb, ty.w0, ty.w1);
                mk[e] = vertical_pass(m0[a] * wa + m0[b] * wb, m1[a] * wa + m1[b] * wb, ty.w0, ty.w1) ? 255 : 0;
            }
        }
        draw_store_dwords<3>(cimg + (size_t)y * C2 * 3, [&](int i) { return px[i]; });  // 4-byte aligned: offsets, S and x0 are multiples of 4
        draw_store_dwords<1>(cmsk + (size_t)y * C2, [&](int i) { return mk[i]; });
    }
}

hipError_t launch_mosaic(unsigned char *base, const hh_mosaic_desc *descs, int n, int S, hipStream_t s)
{
    const int xtiles = (S + MOSAIC_TX * MOSAIC_PX - 1) / (MOSAIC_TX * MOSAIC_PX), ytiles = (S + MOSAIC_TY * MOSAIC_ROWS - 1) / (MOSAIC_TY * MOSAIC_ROWS);
    hipLaunchKernelGGL(mosaic_kernel, dim3(xtiles * ytiles, 4, n), dim3(MOSAIC_TX * MOSAIC_TY), 0, s, base, descs, S, xtiles);
    return hipGetLastError();
}
