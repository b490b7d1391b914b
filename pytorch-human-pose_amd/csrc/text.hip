// Text labels on the GPU: put_txt of the reference (utils/image.py:64-119) for a batch of uint8 [h,w,3] frames of mixed sizes in ONE
// launch, in place, on the frames where the render and resize launches left them.  The rule (the two primitive kinds, their pixel
// arithmetic, the order) is stated at hh_text_labels_u8_batch in include/hhrnet.h; its arithmetic is text_math.h, shared with the
// host.  The host forms the primitive table (keypoints/text.py layout_put_txt), one descriptor per frame and the list of the tiles
// that some primitive touches (text_list_tiles): work scales with the labelled area, not with the frame.
//
// text_labels_kernel: a workgroup of 256 threads owns one listed TEXT_TH x TEXT_TW = 16 x 64 tile of one frame, a thread TEXT_PX = 4
// horizontally adjacent pixels of it (draw_dev.h: draw_tile).  The frame's primitives are walked TEXT_CHUNK = 256 at a time: each
// lane tests one primitive's box against the tile, the survivors are compacted into LDS in draw order (draw_dev.h: draw_cull_slot),
// and every thread walks that list, all lanes reading the same entry at the same time (an LDS broadcast).  A thread keeps its
// pixels in registers across the list and across chunks, so the draw order holds
// within and across chunks and the list never needs more than one chunk of room (8 KB).  A pixel is loaded when the first primitive
// that covers it is applied and stored at the end only if it was loaded: a pixel that no primitive covers is neither read nor
// written, and every covered byte is written exactly once by exactly one thread (the tile list names no tile twice).  Frames are
// tightly packed, any alignment: dword loads and stores where a primitive covers all four pixels of a thread and their 12 bytes are
// 4-byte aligned, bytes otherwise.  The coverage bytes are read from global memory: 30 KB for the whole atlas, a glyph's rows are
// adjacent bytes read by adjacent lanes.
#include "kernels.h"
#include "draw_dev.h"
#include "text_math.h"

#define TEXT_WAVES (TEXT_THREADS / 64)

__global__ __launch_bounds__(TEXT_THREADS) void text_labels_kernel(unsigned char *base, const TextDesc *__restrict__ descs, const TextPrim *__restrict__ prims,
                                                                   const uint8_t *__restrict__ atlas, const TextTile *__restrict__ tiles)
{
    __shared__ TextPrim list[TEXT_CHUNK];
    __shared__ int wave_count[TEXT_WAVES];
    const TextTile listed = tiles[blockIdx.x];
    const TextDesc d = descs[listed.frame];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const DrawTile t = draw_tile(listed.tile, text_xtiles(d.w), d.h, d.w, tid);  // inside the frame: checked on the host
    const int tx0 = t.tx0, ty0 = t.ty0, tx1 = t.tx1, ty1 = t.ty1, y = t.y, x = t.x, npx = t.npx;
    // y < h and x + e < w for e < npx, so every byte touched below is inside the frame's h * w * 3
    unsigned char *ptr = base + d.src_offset + ((size_t)(npx > 0 ? y : 0) * d.w + (npx > 0 ? x : 0)) * 3;
    const bool wide = npx == TEXT_PX && ((uintptr_t)ptr & 3) == 0;
    uint32_t px[TEXT_PX];  // r | g << 8 | b << 16 of the pixels loaded so far
#pragma unroll
    for (int e = 0; e < TEXT_PX; ++e) px[e] = 0;
    unsigned loaded = 0;

    for (int chunk = 0; chunk < d.prim_count; chunk += TEXT_CHUNK) {  // (uniform over the workgroup)
        const int i = chunk + tid;
        TextPrim mine;
        bool keep = false;
        if (i < d.prim_count) {  // prim_offset + i < the table's length: checked on the host
            mine = prims[d.prim_offset + i];
            keep = render_box_meets(mine, tx0, ty0, tx1, ty1);
        }
        const DrawSlot cull = draw_cull_slot<TEXT_WAVES>(keep, lane, wave, wave_count);
        if (keep) list[cull.slot] = mine;  // < cull.total <= TEXT_CHUNK
        __syncthreads();
        if (npx > 0)
            for (int k = 0; k < cull.total; ++k) {
                const TextPrim p = list[k];
                if (y < p.y0 || y > p.y1 || x + npx - 1 < p.x0 || x > p.x1) continue;
                unsigned hit = 0;
#pragma unroll
                for (int e = 0; e < TEXT_PX; ++e) hit |= (e < npx && x + e >= p.x0 && x + e <= p.x1) ? 1u << e : 0u;
                const unsigned need = hit & ~loaded;
                if (need == (1u << TEXT_PX) - 1u && wide) {
                    const DrawPx4 q = draw_load_px4(ptr);
#pragma unroll
                    for (int e = 0; e < TEXT_PX; ++e) px[e] = q.v[e];
                } else if (need) {
#pragma unroll
                    for (int e = 0; e < TEXT_PX; ++e)
                        if (need >> e & 1) px[e] = draw_load_px(ptr + e * 3);
                }
                loaded |= need;
#pragma unroll
                for (int e = 0; e < TEXT_PX; ++e)
                    if (hit >> e & 1) px[e] = text_apply(p, atlas, x + e, y, px[e]);
            }
        __syncthreads();  // the next chunk overwrites the list and the counts
    }
    if (!loaded) return;
    if (loaded == (1u << TEXT_PX) - 1u && wide) {
        draw_store_px4(ptr, [&](int e) { return px[e]; });
    } else {
#pragma unroll
        for (int e = 0; e < TEXT_PX; ++e)
            if (loaded >> e & 1) draw_store_px(ptr + e * 3, px[e]);
    }
}

hipError_t launch_text_labels(unsigned char *base, const TextDesc *descs, const TextPrim *prims, const uint8_t *atlas, const void *tiles, long long num_tiles,
                              hipStream_t s)
{
    hipLaunchKernelGGL(text_labels_kernel, dim3((unsigned)num_tiles), dim3(TEXT_THREADS), 0, s, base, descs, prims, atlas, static_cast<const TextTile *>(tiles));
    return hipGetLastError();
}

void text_debug_host(unsigned char *frame, const TextDesc &d, const TextPrim *prims, const uint8_t *atlas, const void *tiles, long long num_tiles)
{
    TextPrim list[TEXT_CHUNK];
    for (long long i = 0; i < num_tiles; ++i) text_tile_host(frame, d, prims, atlas, static_cast<const TextTile *>(tiles)[i].tile, list);
}
