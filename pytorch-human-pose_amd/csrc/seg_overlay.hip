// Segmentation overlays on the GPU: the per-object cv2.fillPoly + cv2.drawContours + addWeighted of the reference's plot_raw
// (keypoints/datasets/coco.py:383-398) for a batch of uint8 [h,w,3] frames of mixed sizes in ONE launch.  The rule (fill predicate,
// line rule, draw order, blend) is stated at hh_seg_overlay_u8_batch in include/hhrnet.h; its arithmetic is seg_overlay_math.h, shared
// with the host.  The work is render.hip's walk with crowd_mask.hip's transposition in the middle.
//
// seg_overlay_kernel: a workgroup of 256 threads owns one SEG_TH x SEG_TW = 32 x 128 tile of one frame.
// Phase 1, column-wise: thread t owns SEG_ROWS = 16 rows of tile column t % 128 and keeps their overlay colours (SEG_COVERED | colour,
// or 0) in 16 registers.  The frame's shapes are walked SEG_CHUNK = 256 at a time: each lane tests one shape against the tile, the
// survivors are compacted into LDS in draw order (draw_dev.h: draw_cull_slot), and every thread walks that list, all lanes reading
// the same entry at the same time (an LDS broadcast).  A shape gives a thread the bitmask of its rows that it covers: a fill by one upper-bound search in its toggles and a
// cursor down the column (crowd_column_bits: column-major toggles, a lane per column), a line by its exact int64 rule, solved for the
// column.  The registers persist across the list and across chunks, so the draw order holds within and across chunks, no thread ever
// writes another thread's pixel, and the walk needs no barrier besides the cull's.
// The transposition: the 16 colours go to LDS, own[row][column] with a pitch of 132 dwords; the 64 lanes of a wave store 64 consecutive
// dwords (conflict-free under the 32-bank rule of ds_write_b32: each half-wave hits 32 different banks).
// Phase 2, row-wise: a half-wave owns a tile row at a time, a lane SEG_PX = 4 adjacent pixels = 12 bytes of it.  Frames carry no
// alignment guarantee, so per row `head` = the 0..3 pixels in front of the first 4-byte-aligned 12-byte group is taken from the
// destination row's address ((address + 3 p) % 4 == 0 iff p % 4 == address % 4); the head pixels and a ragged tail go as bytes,
// everything between as three dwords per lane, loaded the same way when the source row has the destination's alignment (always so in
// place).  A lane reads its eight candidate colours from LDS as two aligned ds_read_b128 (consecutive lanes on consecutive 16-byte
// slots) and picks four by `head`.  Every output byte is written exactly once by exactly one lane, every source byte is read by the
// lane that writes its pixel (so dst may be src); no atomics; nothing depends on the launch.
#include "kernels.h"
#include "draw_dev.h"
#include "seg_overlay_math.h"

#define SEG_WAVES (SEG_THREADS / 64)

__global__ __launch_bounds__(SEG_THREADS) void seg_overlay_kernel(unsigned char *base, const SegDesc *__restrict__ descs, const SegShape *__restrict__ shapes,
                                                                  const uint32_t *__restrict__ toggles)
{
    __shared__ SegItem list[SEG_CHUNK];
    __shared__ int wave_count[SEG_WAVES];
    __shared__ __attribute__((aligned(16))) uint32_t own_lds[SEG_TH * SEG_PITCH];
    const SegDesc d = descs[blockIdx.y];
    const int xtiles = (d.w + SEG_TW - 1) / SEG_TW, ytiles = (d.h + SEG_TH - 1) / SEG_TH;
    if ((int)blockIdx.x >= xtiles * ytiles) return;  // the grid is sized for the largest frame; uniform over the workgroup
    const int tx0 = ((int)blockIdx.x % xtiles) * SEG_TW, ty0 = ((int)blockIdx.x / xtiles) * SEG_TH;
    const int ty1 = min(ty0 + SEG_TH, d.h) - 1, tx1 = min(tx0 + SEG_TW, d.w) - 1;  // inside the frame
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- phase 1: thread = (column, SEG_ROWS rows)
    const int col = tid % SEG_TW, seg = tid / SEG_TW;
    const int X = tx0 + col, Y0 = ty0 + seg * SEG_ROWS;
    const int myrows = X <= tx1 ? min(SEG_ROWS, ty1 - Y0 + 1) : 0;  // <= 0: no pixel of this thread is inside the frame
    uint32_t own[SEG_ROWS];
#pragma unroll
    for (int r = 0; r < SEG_ROWS; ++r) own[r] = 0u;

    for (int chunk = 0; chunk < d.prim_count; chunk += SEG_CHUNK) {  // (uniform over the workgroup)
        const int i = chunk + tid;
        SegItem mine;
        bool keep = false;
        if (i < d.prim_count) {  // prim_offset + i < the table's length: checked on the host
            const SegShape s = shapes[d.prim_offset + i];
            keep = seg_meets(s, tx0, ty0, tx1, ty1);
            mine = seg_item(s);
        }
        const DrawSlot cull = draw_cull_slot<SEG_WAVES>(keep, lane, wave, wave_count);
        if (keep) list[cull.slot] = mine;  // < cull.total <= SEG_CHUNK
        __syncthreads();
        if (myrows > 0)
            for (int k = 0; k < cull.total; ++k) {
                const SegItem s = list[k];
                // X < w and Y0 + myrows <= h: a fill's searches stay inside its own toggles (range checked on the host)
                const uint32_t bits = seg_item_bits(s, toggles, d.h, X, Y0, myrows);
                if (!bits) continue;
                const uint32_t v = SEG_COVERED | (uint32_t)s.colour;
#pragma unroll
                for (int r = 0; r < SEG_ROWS; ++r) own[r] = (bits >> r & 1) ? v : own[r];
            }
        __syncthreads();  // the next chunk overwrites the list and the counts
    }

    // ---- the transposition: own_lds[row][column]; the SEG_PX pad columns of a row are read by the last lane's second read, never used
#pragma unroll
    for (int r = 0; r < SEG_ROWS; ++r) own_lds[(seg * SEG_ROWS + r) * SEG_PITCH + col] = own[r];
    if (tid < SEG_TH * SEG_PX) own_lds[(tid / SEG_PX) * SEG_PITCH + SEG_TW + tid % SEG_PX] = 0u;
    __syncthreads();

    // ---- phase 2: half-wave = a tile row, lane = SEG_PX pixels
    const int cols = tx1 - tx0 + 1, rows = ty1 - ty0 + 1;
    const int g = tid & 31;
    const float w0 = d.w0, w1 = d.w1;
    const int flags = d.flags;
    for (int r = tid >> 5; r < rows; r += SEG_THREADS / 32) {
        const size_t at = ((size_t)(ty0 + r) * d.w + tx0) * 3;  // + 3 * cols <= h * w * 3: inside the frame
        const unsigned char *srow = base + d.src_offset + at;
        unsigned char *drow = base + d.dst_offset + at;
        const int head = (int)(reinterpret_cast<uintptr_t>(drow) & 3);
        const bool src_aligned = ((reinterpret_cast<uintptr_t>(srow) ^ reinterpret_cast<uintptr_t>(drow)) & 3) == 0;
        const uint32_t *orow = &own_lds[r * SEG_PITCH];
        if (g < head && g < cols) draw_store_px(drow + 3 * g, seg_pixel(draw_load_px(srow + 3 * g), orow[g], w0, w1, flags));
        const int p0 = head + SEG_PX * g;  // the tile column of this lane's first pixel; columns from `cols` on are not this tile's
        if (p0 >= cols) continue;
        const uint4 qa = *reinterpret_cast<const uint4 *>(&orow[SEG_PX * g]), qb = *reinterpret_cast<const uint4 *>(&orow[SEG_PX * g + 4]);
        uint32_t o0, o1, o2, o3;
        switch (head) {
        case 0: o0 = qa.x, o1 = qa.y, o2 = qa.z, o3 = qa.w; break;
        case 1: o0 = qa.y, o1 = qa.z, o2 = qa.w, o3 = qb.x; break;
        case 2: o0 = qa.z, o1 = qa.w, o2 = qb.x, o3 = qb.y; break;
        default: o0 = qa.w, o1 = qb.x, o2 = qb.y, o3 = qb.z; break;
        }
        const unsigned char *sp = srow + 3 * p0;
        unsigned char *dp = drow + 3 * p0;  // 4-byte aligned by the choice of head
        if (p0 + SEG_PX <= cols) {
            uint32_t s[SEG_PX];
            if (src_aligned) {
                const DrawPx4 q = draw_load_px4(sp);
                s[0] = q.v[0], s[1] = q.v[1], s[2] = q.v[2], s[3] = q.v[3];
            } else {
                s[0] = draw_load_px(sp), s[1] = draw_load_px(sp + 3), s[2] = draw_load_px(sp + 6), s[3] = draw_load_px(sp + 9);
            }
            const uint32_t r[SEG_PX] = {seg_pixel(s[0], o0, w0, w1, flags), seg_pixel(s[1], o1, w0, w1, flags), seg_pixel(s[2], o2, w0, w1, flags),
                                        seg_pixel(s[3], o3, w0, w1, flags)};
            draw_store_px4(dp, [&](int e) { return r[e]; });
        } else {
            const uint32_t o[SEG_PX] = {o0, o1, o2, o3};
#pragma unroll
            for (int e = 0; e < SEG_PX; ++e)
                if (p0 + e < cols) draw_store_px(dp + 3 * e, seg_pixel(draw_load_px(sp + 3 * e), o[e], w0, w1, flags));
        }
    }
}

hipError_t launch_seg_overlay(unsigned char *base, const hh_seg_desc *descs, const int32_t *shapes, const unsigned int *toggles, int n, int max_tiles, hipStream_t s)
{
    hipLaunchKernelGGL(seg_overlay_kernel, dim3(max_tiles, n), dim3(SEG_THREADS), 0, s, base, descs, reinterpret_cast<const SegShape *>(shapes), toggles);
    return hipGetLastError();
}
